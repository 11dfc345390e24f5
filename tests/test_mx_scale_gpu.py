"""GPU: `--mx_scale_search` on the device — k_mx_scale_search_rows / _cols (dpl_mx_scale_search) and the given-scale forms of the Q/DQ
and encode kernels (dpl_fake_quant_mx_scaled, dpl_mx_encode_scaled) — against the numpy definition (tests/mx_scale_model.py):
bytes by equality, `err` and y as bit patterns, NaN in the same places, guard bands around every output untouched.  No tolerance
anywhere but where the block-scaled matrix instruction sums (the bound of tests/test_mx_gemm_gpu.py).  Shapes are the smallest
that reach every path: inner == 1 runs 8 lanes per block on 16-byte vectors when x is 16-byte aligned and K % 4 == 0 and 32 lanes
per block otherwise (a workgroup owns 128 or 32 blocks: 67 rows of 96 are 201), inner > 1 gives a lane four columns when
inner % 4 == 0 and x is aligned, else one; each form sums the 32 squared errors of a block through different lanes."""
import ctypes as C
import gc
import types

import numpy as np
import pytest
import torch

import mx_gemm_model as G
import mx_model as M
import mx_pack_model as P
import mx_scale_model as S

pytestmark = pytest.mark.gpu

ELEMS = ("mxfp8", "mxfp4")
CODE = {"mxfp8": 0, "mxfp4": 1}
GUARD = 64          # bytes around every output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _lines(n, k, seed):
    """n fibres of k elements, in turn N(0, 1), U(-1, 1) * 2^e and E4M3 tie lines (values on the E4M3 grid under either exponent:
    both errors 0), a few exact zeros of both signs and fp32 subnormals among them — so that both choices occur."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, k), np.float32)
    for r in range(n):
        if r % 3 == 0:
            x[r] = rng.standard_normal(k)
        elif r % 3 == 1:
            x[r] = np.ldexp(rng.uniform(-1, 1, k), int(rng.integers(-30, 30)))
        else:
            x[r] = np.ldexp(rng.choice([1.0, -1.0, 1.5, 2.0, -3.0, 0.5, 0.25, 4.0], k), int(rng.integers(-5, 5)))
    flat = x.reshape(-1)
    flat[7::37] = 0.0
    flat[5::91] = -0.0
    flat[11::113] = np.float32(1e-41)
    return x


def _tensor(outer, k, inner, seed):
    """[outer, k, inner] whose fibres along k are _lines."""
    return np.ascontiguousarray(_lines(outer * inner, k, seed).reshape(outer, inner, k).transpose(0, 2, 1))


def _same(got, want, what):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32))))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _placed(x, dev, off):
    """x on the device at a base that is 16-byte aligned (off = 0) or one float past it."""
    buf = torch.zeros(x.size + 4 + off, dtype=torch.float32, device=dev)
    v = buf[off:off + x.size].view(x.shape)
    assert v.data_ptr() % 16 == 4 * off
    v.copy_(torch.from_numpy(x))
    return v


class _Guarded:
    """n elements of `dtype` on the device between two guard bands of GUARD bytes; the view starts on a 16-byte boundary."""

    def __init__(self, n, dtype, fill, dev):
        self.g = GUARD // torch.empty((), dtype=dtype).element_size()
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * self.g,), fill, dtype=dtype, device=dev)
        self.view = self.buf[self.g:self.g + n]
        assert self.view.data_ptr() % 16 == 0

    def host(self, what):
        """The n elements; asserts that nothing around them was written."""
        h = self.buf.cpu().numpy()
        assert (h[:self.g] == self.fill).all() and (h[self.g + self.n:] == self.fill).all(), (what, "written outside the output")
        return h[self.g:self.g + self.n]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(x, axis, dev, what, off=0):
    """Every claim of this file on one tensor, per element type.  -> per element type, did (some block move up, some block stay)."""
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    axis, outer, k, inner = P._split(x.shape, axis)
    nblk = -(-k // 32)
    nb = outer * nblk * inner
    rng = np.random.default_rng(x.size)
    seen = {}
    for elem in ELEMS:
        want_s, want_err = S.scale_search(x, axis, elem)
        floor = S.floor_scales(x, axis, elem)
        xv = _placed(x, dev, off)
        # the search: bytes and both errors, through the C ABI into guarded buffers, with and without err
        gs, ge = _Guarded(nb, torch.uint8, 0xA5, dev), _Guarded(2 * nb, torch.float64, -77.0, dev)
        assert lib.dpl_mx_scale_search(CODE[elem], _ptr(xv), outer, k, inner, _ptr(gs.view), _ptr(ge.view), _stream()) == 0
        torch.cuda.synchronize()
        hs, he = gs.host((what, elem, "scales")), ge.host((what, elem, "err"))
        assert np.array_equal(hs, want_s.reshape(-1)), (what, elem, off, "bytes", np.flatnonzero(hs != want_s.reshape(-1))[:5])
        assert np.array_equal(he.view(np.uint64), want_err.reshape(-1).view(np.uint64)), (what, elem, off, "err")
        block_shape = tuple(x.shape[:axis]) + (nblk,) + tuple(x.shape[axis + 1:])
        s_dev = ops.mx_scale_search(xv, axis, elem)
        assert s_dev.dtype == torch.uint8 and tuple(s_dev.shape) == block_shape
        assert np.array_equal(s_dev.cpu().numpy().reshape(-1), hs), (what, elem, off, "without err")
        seen[elem] = (bool((want_s != floor).any()), bool((want_s == floor).any()))
        # the given-scale pair under the searched bytes, random bytes and the floor's
        for name, s in (("searched", want_s), ("random", rng.integers(0, 256, want_s.shape).astype(np.uint8)), ("floor", floor)):
            tag = (what, elem, off, name)
            sd = torch.from_numpy(np.ascontiguousarray(s)).to(dev).view(block_shape)
            want_y, eff = S.fake_quant_mx_scaled(x, axis, elem, s, return_scales=True)
            gy = _Guarded(x.size + off, torch.float32, -77.0, dev)
            yv = gy.view[off:].view(x.shape)
            assert ops.fake_quant_mx_scaled(xv, axis, elem, sd, out=yv) is yv
            got_y = gy.host(tag)[off:]
            if off:
                assert (gy.host(tag)[:off] == -77.0).all(), tag
            _same(got_y, want_y, tag + ("y",))
            xin = _placed(x, dev, off)                                        # in place
            ops.fake_quant_mx_scaled(xin, axis, elem, sd, out=xin)
            _same(xin.cpu().numpy(), want_y, tag + ("in place",))
            if name == "floor":
                _same(got_y, ops.fake_quant_mx(xv, axis, elem).cpu().numpy(), tag + ("fake_quant_mx",))
            want_c, want_ps = S.encode_scaled(x, axis, elem, s)
            gc_, gp = _Guarded(want_c.size, torch.uint8, 0xA5, dev), _Guarded(want_ps.size, torch.uint8, 0xA5, dev)
            assert lib.dpl_mx_encode_scaled(CODE[elem], _ptr(xv), outer, k, inner, _ptr(sd), _ptr(gc_.view), _ptr(gp.view), _stream()) == 0
            torch.cuda.synchronize()
            hc, hp = gc_.host(tag + ("codes",)), gp.host(tag + ("packed scales",))
            assert np.array_equal(hc, want_c.reshape(-1)), tag + ("codes", np.flatnonzero(hc != want_c.reshape(-1))[:5])
            assert np.array_equal(hp, want_ps.reshape(-1)), tag + ("packed scales",)
            assert np.array_equal(hp.reshape(outer, inner, nblk), eff.transpose(0, 2, 1)), tag      # the given bytes transposed, 0xFF ...
            codes, packed = ops.mx_encode_scaled(xv, axis, elem, sd)
            assert np.array_equal(codes.cpu().numpy(), want_c) and np.array_equal(packed.cpu().numpy(), want_ps), tag
            _same(ops.mx_decode(codes, packed, elem, x.shape, axis).cpu().numpy(), got_y, tag + ("decode(encode_scaled)",))
    return seen


def _both(seen):
    for elem in ELEMS:
        assert any(s[elem][0] for s in seen) and any(s[elem][1] for s in seen), (elem, "both choices must occur")


# ------------------------------------------------------------------------------------------------ 1. contiguous blocks
@pytest.mark.parametrize("k", [1, 4, 31, 32, 33, 36, 96, 100])
def test_rows_path(dev, k):
    seen = []
    for outer in (1, 3, 67):
        x = _tensor(outer, k, 1, 1000 * outer + k).reshape(outer, k)
        seen.append(_check(x, 1, dev, (outer, k)))
        seen.append(_check(x, 1, dev, (outer, k, "one float off"), off=1))       # the element-by-element form
    _both(seen)


# ------------------------------------------------------------------------------------------------ 2. strided blocks
@pytest.mark.parametrize("shape,axis", [((3, 70, 4), -2),     # four columns to a lane, a short last block
                                        ((2, 40, 17), -2),    # odd inner: one column to a lane
                                        ((1, 64, 64), -2),    # 32 slots of four columns / 128 blocks
                                        ((2, 33, 3), -2),     # a last block of one row
                                        ((40, 6), 0),         # outer == 1 along axis 0
                                        ((2, 160, 68), 1)])   # the encoder's tiles of 4 K-blocks x 16 column groups: 5 and 17
def test_cols_path(dev, shape, axis):
    outer, k, inner = (1,) + shape if len(shape) == 2 else shape
    x = _tensor(outer, k, inner, 100000 * outer + 1000 * k + inner).reshape(shape)
    _both([_check(x, axis, dev, shape)])


# ------------------------------------------------------------------------------------------------ 3. special values
def _special_rows():
    """[9, 64]: block 0 of every row is special, block 1 ordinary."""
    ordinary = np.linspace(-3, 3, 32).astype(np.float32)
    x = np.tile(ordinary, (9, 2)).astype(np.float32)
    x[0, 7] = np.nan                                       # a NaN block
    x.view(np.uint32)[0, 9] = 0xFFC00001
    x[1, 9] = np.inf                                       # an inf block
    x[2, 11] = -np.inf
    x[3, :32] = 0
    x[3, 1:32:2] = -0.0                                    # all zero, -0 among them: the Q/DQ keeps the signs
    x[4, :32] = np.float32(2.0 ** -131)
    x[4, 0] = -np.float32(2.0 ** -130)                     # the maximum is an fp32 subnormal: se0 = -127
    x[4, 5] = np.float32(1.875 * 2.0 ** -131)
    x[5, :32] = np.float32(2.0 ** -127)
    x[5, 3] = np.float32(2.0 ** -120)                      # subnormal values under se0 = -127 (E4M3)
    x[5, 4] = np.float32(1.9 * 2.0 ** -120)
    x[6, :32] = np.float32(1.0)
    x[6, 31] = np.float32(3.4028234663852886e38)           # the fp32-max block: no upper candidate
    x[7, :32] = np.float32(-3.4028234663852886e38)
    x[8, :32] = np.linspace(-7.9, 7.9, 32)                 # moves up under either format
    return x


def test_special_values(dev):
    x = _special_rows()
    for elem in ELEMS:
        s, err = S.scale_search(x, 1, elem)
        top = 127 - M.EMAX[elem] + 127
        assert s[:3, 0, 0].tolist() == [0xFF] * 3 and np.isposinf(err[:3, 0]).all()
        assert s[3, 0, 0] == 0 and err[3, 0].reshape(-1).tolist() == [0.0, 0.0]
        assert s[4, 0, 0] in (0, 1) and S.floor_scales(x, 1, elem)[4:6, 0, 0].tolist() == [0, 0 if elem == "mxfp8" else 5]
        assert s[6, 0, 0] == s[7, 0, 0] == top and err[6, 0, 0, 0] == err[6, 0, 0, 1]
        assert s[8, 0, 0] == S.floor_scales(x, 1, elem)[8, 0, 0] + 1
        y = S.fake_quant_mx_scaled(x, 1, elem, s)
        assert np.array_equal(np.signbit(y[3, :32]), np.signbit(x[3, :32])) and (y[3, :32] == 0).all()
    for off in (0, 1):
        _check(x, 1, dev, "rows", off)
        _check(np.ascontiguousarray(x.T), 0, dev, "columns", off)      # the same blocks strided: four columns to a lane, then one
    _check(np.ascontiguousarray(x[:, :63].T), 0, dev, "columns, inner 9, K 63")


# ------------------------------------------------------------------------------------------------ 4. entry points
def test_entry_points(dev):
    import dipoorlet_amd.torch_ops  # noqa: F401
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    xh = _tensor(3, 40, 6, 3)
    x = torch.from_numpy(xh).to(dev)
    st = _stream()
    for elem in ELEMS:
        for axis in (0, 1, 2, -1, -2, -3):
            want_s, want_err = S.scale_search(xh, axis, elem)
            a = axis % 3
            shape = tuple(-(-d // 32) if i == a else d for i, d in enumerate(xh.shape))
            err = torch.empty(shape + (2,), dtype=torch.float64, device=dev)
            s = ops.mx_scale_search(x, axis, elem, err=err)
            assert tuple(s.shape) == shape and np.array_equal(s.cpu().numpy().reshape(-1), want_s.reshape(-1)), (elem, axis)
            assert np.array_equal(err.cpu().numpy().reshape(-1).view(np.uint64), want_err.reshape(-1).view(np.uint64)), (elem, axis)
            ts = torch.ops.dipoorlet.mx_scale_search(x, axis, elem)
            assert torch.equal(ts, s), ("torch op", elem, axis)
            y = ops.fake_quant_mx_scaled(x, axis, elem, s)
            _same(y.cpu().numpy(), S.fake_quant_mx_scaled(xh, axis, elem, want_s), (elem, axis))
            ty = torch.ops.dipoorlet.fake_quant_mx_scaled(x, axis, elem, s)
            assert torch.equal(ty.view(torch.int32), y.view(torch.int32)), ("torch op", elem, axis)
    xt = x.transpose(0, 2)              # (the torch ops make their inputs contiguous, as their siblings do)
    ts = torch.ops.dipoorlet.mx_scale_search(xt, 1, "mxfp4")
    assert np.array_equal(ts.cpu().numpy().reshape(-1), S.scale_search(xt.contiguous().cpu().numpy(), 1, "mxfp4")[0].reshape(-1))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fx = torch.empty(5, 49, 3, device="cuda")
        fs = torch.ops.dipoorlet.mx_scale_search(fx, 1, "mxfp4")
        assert tuple(fs.shape) == (5, 2, 3) and fs.dtype == torch.uint8
        fy = torch.ops.dipoorlet.fake_quant_mx_scaled(fx, -2, "mxfp8", fs)
        assert tuple(fy.shape) == (5, 49, 3) and fy.dtype == torch.float32
    # the Python checks
    s = ops.mx_scale_search(x, 1, "mxfp8")
    assert ops.mx_scale_search(torch.empty(0, 5, device=dev), 1, "mxfp8").shape == (0, 1)
    e = torch.empty(0, 5, device=dev)
    assert ops.fake_quant_mx_scaled(e, 1, "mxfp8", torch.empty(0, 1, dtype=torch.uint8, device=dev)).shape == (0, 5)
    ec, es = ops.mx_encode_scaled(e, 1, "mxfp8", torch.empty(0, 1, dtype=torch.uint8, device=dev))
    assert tuple(ec.shape) == (0, 32) and tuple(es.shape) == (0, 1)
    for bad in (dict(elem="mxfp6"), dict(axis=3), dict(axis=-4), dict(axis=None)):
        kw = dict(axis=1, elem="mxfp8")
        kw.update(bad)
        for fn in (lambda: ops.mx_scale_search(x, kw["axis"], kw["elem"]), lambda: ops.fake_quant_mx_scaled(x, kw["axis"], kw["elem"], s),
                   lambda: ops.mx_encode_scaled(x, kw["axis"], kw["elem"], s)):
            with pytest.raises(_hip.DipoorletHipError, match="'mxfp8' or 'mxfp4'" if "elem" in bad else "axis"):
                fn()
    for fn in (lambda: ops.mx_scale_search(x.transpose(0, 1), 1, "mxfp8"), lambda: ops.mx_scale_search(x.cpu(), 1, "mxfp8"),
               lambda: ops.mx_scale_search(x, 1, "mxfp8", err=torch.empty(3, 2, 6, 2, device=dev)),                  # fp32 err
               lambda: ops.mx_scale_search(x, 1, "mxfp8", err=torch.empty(3, 2, 6, dtype=torch.float64, device=dev)),
               lambda: ops.fake_quant_mx_scaled(x, 1, "mxfp8", s.cpu()), lambda: ops.fake_quant_mx_scaled(x, 1, "mxfp8", s.to(torch.int32)),
               lambda: ops.fake_quant_mx_scaled(x, 1, "mxfp8", s[:, :1].contiguous()),
               lambda: ops.fake_quant_mx_scaled(x, 1, "mxfp8", s, out=torch.empty(3, 40, 5, device=dev)),
               lambda: ops.mx_encode_scaled(x, 1, "mxfp8", s[:, :, :5].contiguous()), lambda: ops.mx_encode_scaled(x.cpu(), 1, "mxfp8", s)):
        with pytest.raises(_hip.DipoorletHipError):
            fn()
    # the C ABI: every refusal returns -2 with its message and launches nothing
    codes = torch.full((3 * 6 * 64 + 32,), 0xA5, dtype=torch.uint8, device=dev)
    packed = torch.full((3 * 6 * 2,), 0xA5, dtype=torch.uint8, device=dev)
    sc = torch.full((3 * 2 * 6,), 0xA5, dtype=torch.uint8, device=dev)
    er = torch.full((3 * 2 * 6 * 2,), -77.0, dtype=torch.float64, device=dev)
    y = torch.full((3 * 40 * 6,), -77.0, dtype=torch.float32, device=dev)
    px, py, pc, pp, ps, pe, pg = (_ptr(t) for t in (x, y, codes, packed, sc, er, s))
    for elem in (2, -1):
        assert lib.dpl_mx_scale_search(elem, px, 3, 40, 6, ps, pe, st) == -2 and b"dpl_mx_scale_search: elem" in lib.dpl_last_error()
        assert lib.dpl_fake_quant_mx_scaled(elem, px, py, 3, 40, 6, pg, st) == -2 and b"dpl_fake_quant_mx_scaled: elem" in lib.dpl_last_error()
        assert lib.dpl_mx_encode_scaled(elem, px, 3, 40, 6, pg, pc, pp, st) == -2 and b"dpl_mx_encode_scaled: elem" in lib.dpl_last_error()
    assert lib.dpl_mx_scale_search(0, None, 3, 40, 6, ps, pe, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_scale_search(0, px, 3, 40, 6, None, pe, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx_scaled(0, None, py, 3, 40, 6, pg, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx_scaled(0, px, None, 3, 40, 6, pg, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx_scaled(0, px, py, 3, 40, 6, None, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_encode_scaled(0, None, 3, 40, 6, pg, pc, pp, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_encode_scaled(0, px, 3, 40, 6, None, pc, pp, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_encode_scaled(0, px, 3, 40, 6, pg, None, pp, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_encode_scaled(0, px, 3, 40, 6, pg, pc, None, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_scale_search(0, px, 1, 1 << 31, 1, ps, pe, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_mx_scale_search(0, px, 1, 1, 1 << 31, ps, pe, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx_scaled(1, px, py, 1, 1 << 31, 1, pg, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx_scaled(1, px, py, 1, 1, 1 << 31, pg, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_mx_encode_scaled(1, px, 1, 1 << 31, 1, pg, pc, pp, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_mx_encode_scaled(1, px, 1, 1, 1 << 31, pg, pc, pp, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_mx_scale_search(0, px, 1 << 40, 1 << 20, 1 << 20, ps, pe, st) == -2 and b"too large" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx_scaled(0, px, py, 1 << 40, 1 << 20, 1 << 20, pg, st) == -2 and b"too large" in lib.dpl_last_error()
    assert lib.dpl_mx_encode_scaled(0, px, 1 << 40, 1 << 20, 1 << 20, pg, pc, pp, st) == -2 and b"too large" in lib.dpl_last_error()
    assert lib.dpl_mx_encode_scaled(1, px, 1 << 58, 1, 1, pg, pc, pp, st) == -2 and b"too large" in lib.dpl_last_error()      # (32 pad codes per row)
    for shift in (1, 4, 8):
        mis = C.c_void_p(codes.data_ptr() + shift)
        assert lib.dpl_mx_encode_scaled(0, px, 3, 40, 6, pg, mis, pp, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
    for zero in ((0, 40, 6), (3, 0, 6), (3, 40, 0)):       # n == 0: a no-op, whatever the pointers
        assert lib.dpl_mx_scale_search(1, None, *zero, None, None, st) == 0
        assert lib.dpl_fake_quant_mx_scaled(1, None, None, *zero, None, st) == 0
        assert lib.dpl_mx_encode_scaled(1, None, *zero, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert (codes == 0xA5).all() and (packed == 0xA5).all() and (sc == 0xA5).all() and (er == -77.0).all() and (y == -77.0).all()
    assert torch.equal(s, ops.mx_scale_search(x, 1, "mxfp8")) and torch.equal(x, torch.from_numpy(xh).to(dev))
    # ... and on a boundary the encoder writes its codes and nothing behind them
    assert lib.dpl_mx_encode_scaled(0, px, 3, 40, 6, pg, C.c_void_p(codes.data_ptr() + 16), pp, st) == 0
    torch.cuda.synchronize()
    hb = codes.cpu().numpy()
    want_c, want_p = S.encode_scaled(xh, 1, "mxfp8", s.cpu().numpy())
    assert (hb[:16] == 0xA5).all() and (hb[16 + 3 * 6 * 64:] == 0xA5).all() and np.array_equal(hb[16:16 + 3 * 6 * 64], want_c.reshape(-1))
    assert np.array_equal(packed.cpu().numpy(), want_p.reshape(-1))


# ------------------------------------------------------------------------------------------------ 5. the session
@pytest.mark.parametrize("elem", ELEMS)
def test_session_folds_constants_under_their_searched_scales(dev, elem):
    """MatMul with a constant [64, 48] weight (blocks along axis -2: strided) and Gemm with transB = 1 (blocks along axis 1:
    contiguous), quantised with the flag: the session's folded constants are the model's Q/DQ under the model's searched bytes, and
    the same weights as bytes (mx_encode_scaled) give, through the block-scaled matrix instruction, mx_gemm_model's product."""
    from dipoorlet_amd import ops
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.models import _B
    from dipoorlet_amd.quantize import quant_graph
    b = _B(17)
    m = b.node("MatMul", ["input", b.w("w1", (64, 48), fan_in=64)], out="m")                 # [1, 4, 48]
    f = b.node("Flatten", [m], out="flat", axis=1)                                            # [1, 192]
    out = b.node("Gemm", [f, b.w("wg", (5, 192)), b.b("bg", 5)], out="output", alpha=1.0, beta=1.0, transB=1)
    g = b.finish("input", [1, 4, 64], out)
    clip = {n: [np.float32(-1.0), np.float32(2.0)] for n in ("input", "m", "flat", "output")}
    wg = g.get_initializer("wg")
    clip["wg"] = [wg.min(1), wg.max(1)]
    args = types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx=elem, mx_scale_search=True)
    gq, _ = quant_graph(g, clip, args)
    sess = GraphSession(gq, device=dev)
    rng = np.random.default_rng(2)
    moved = []
    for name, axis in (("w1", -2), ("wg", 1)):
        q = gq._qdq[name + "_QuantizeLinear"]
        w = g.get_initializer(name)
        want_s = S.scale_search(w, axis, elem)[0]
        assert q.is_mx and q.block_axis == axis and q.mx_scales.dtype == np.uint8
        assert np.array_equal(q.mx_scales.reshape(-1), want_s.reshape(-1)) and np.array_equal(gq.initializer[q.scale_name], q.mx_scales)
        moved.append(want_s != S.floor_scales(w, axis, elem))
        assert q.q_name in sess._folded
        _same(sess.consts[q.output].cpu().numpy(), S.fake_quant_mx_scaled(w, axis, elem, want_s), name)
        # as bytes, against an activation of the right length
        wd = torch.from_numpy(w).to(dev)
        w_codes, w_scales = ops.mx_encode_scaled(wd, axis, elem, torch.from_numpy(q.mx_scales).to(dev))
        k = w.shape[axis]
        xa = torch.from_numpy(rng.standard_normal((7, k)).astype(np.float32)).to(dev)
        a_codes, a_scales = ops.mx_encode(xa, -1, elem)
        got = ops.mx_gemm(a_codes, a_scales, w_codes, w_scales, elem).cpu().numpy()
        ref, s_abs = G.mx_gemm(a_codes.cpu().numpy(), a_scales.cpu().numpy(), w_codes.cpu().numpy(), w_scales.cpu().numpy(), elem)
        assert np.array_equal(w_codes.cpu().numpy(), S.encode_scaled(w, axis, elem, want_s)[0])
        bound = G.bound(s_abs, 32 * -(-k // 32), 1.0 if elem == "mxfp4" else G.HW_FACTOR)
        assert not np.isnan(got).any() and (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= bound).all(), name
    assert any(mv.any() for mv in moved) and not all(mv.all() for mv in moved)
    for n in gq.graph.node:                 # an activation's node keeps the floor rule
        if n.op_type == "FakeQuant" and n.input[0] not in g.initializer:
            assert gq._qdq[n.name].mx_scales is None
    assert torch.isfinite(sess.run_named({"input": torch.from_numpy(rng.standard_normal((1, 4, 64)).astype(np.float32)).to(dev)}, [out])[0]).all()
