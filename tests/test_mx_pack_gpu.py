"""GPU: the element-code kernels of `--mx_pack` (k_mx_encode_rows / _cols, k_mx_decode_rows / _cols; dpl_mx_encode, dpl_mx_decode)
against the numpy definition (tests/mx_pack_model.py) byte for byte, and against the Q/DQ kernel they must agree with:
ops.mx_decode(*ops.mx_encode(x)) is ops.fake_quant_mx(x) bit for bit, NaN in the same places, and the scale bytes are
fake_quant_mx's after the axis swap.  No tolerance anywhere in this file.  Shapes are the smallest that reach every path: inner == 1
runs 8 lanes per block on 16-byte vectors when x is 16-byte aligned and K % 4 == 0 and 32 lanes per block otherwise (a workgroup
owns 128 or 32 blocks), inner > 1 gives a lane four columns when inner % 4 == 0 and x is aligned (a wave is a tile of 4 K-blocks by 16 column
groups), else one (a wave is 64 slots); each way the lanes exchange or assemble codes differently before their 16-byte stores."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import mx_model as M
import mx_pack_model as P

pytestmark = pytest.mark.gpu

ELEMS = ("mxfp8", "mxfp4")
GUARD = 64          # bytes (16 floats) around every output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _data(shape, seed):
    """Values over some forty binades, a few exact zeros of both signs and fp32 subnormals among them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 20, shape))).astype(np.float32)
    flat = x.reshape(-1)
    flat[::37] = 0.0
    flat[5::91] = -0.0
    flat[11::113] = np.float32(1e-41)
    return x


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


def _check(x, axis, dev, what, offsets=(0,)):
    """Every claim of this file on one tensor, per element type and per base offset of the fp32 side."""
    from dipoorlet_amd import ops
    for elem in ELEMS:
        want_c, want_s = P.encode(x, axis, elem)
        want_y, qdq_s = M.fake_quant_mx(x, axis, elem, return_scales=True)
        for off in offsets:
            xv = _placed(x, dev, off)
            codes, scales = ops.mx_encode(xv, axis, elem)
            assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
            assert tuple(codes.shape) == want_c.shape and tuple(scales.shape) == want_s.shape, (what, elem)
            hc, hs = codes.cpu().numpy(), scales.cpu().numpy()
            assert np.array_equal(hs, want_s), (what, elem, off, "scales")
            assert np.array_equal(hc, want_c), (what, elem, off, "codes", np.flatnonzero(hc != want_c)[:5])
            # the scale bytes are the Q/DQ kernel's, K-innermost: [outer, nblk, inner] -> [outer, inner, nblk]
            sc = torch.empty(qdq_s.shape, dtype=torch.uint8, device=dev)
            y_qdq = ops.fake_quant_mx(xv, axis, elem, scales=sc)
            assert np.array_equal(sc.cpu().numpy().transpose(0, 2, 1).reshape(-1), hs.reshape(-1)), (what, elem, off, "axis swap")
            # decode into a guarded buffer at the same offset: the Q/DQ kernel's output bit for bit, nothing written around it
            n = x.size
            by = torch.full((n + 2 * (GUARD // 4) + off,), -77.0, dtype=torch.float32, device=dev)
            yv = by[GUARD // 4 + off:GUARD // 4 + off + n].view(x.shape)
            assert ops.mx_decode(codes, scales, elem, x.shape, axis, out=yv) is yv
            hy = by.cpu().numpy()
            assert (hy[:GUARD // 4 + off] == -77.0).all() and (hy[GUARD // 4 + off + n:] == -77.0).all(), (what, elem, off, "written outside y")
            got = hy[GUARD // 4 + off:GUARD // 4 + off + n]
            _same(got, y_qdq.cpu().numpy(), (what, elem, off, "decode(encode) vs fake_quant_mx"))
            _same(got, want_y, (what, elem, off, "decode(encode) vs model"))
            _same(got, P.decode(want_c, want_s, elem, x.shape, axis), (what, elem, off, "decode vs model decode"))


# ------------------------------------------------------------------------------------------------ 1. contiguous blocks
@pytest.mark.parametrize("shape,offsets", [((67, 96), (0,)),      # 201 groups: past a workgroup's 128
                                           ((5, 100), (0,)),      # a short last block on 16-byte vectors
                                           ((4, 33), (0,)),       # K % 4 != 0: element by element, 32 lanes a block
                                           ((3, 31), (0,)),
                                           ((2, 1), (0,)),
                                           ((9, 64), (1,))])      # a base one float off: the element-wise fallback
def test_rows_path(dev, shape, offsets):
    _check(_data(shape, 1000 * shape[0] + shape[1]), 1, dev, shape, offsets)


# ------------------------------------------------------------------------------------------------ 2. strided blocks
@pytest.mark.parametrize("shape,offsets", [((3, 70, 4), (0,)),    # four columns to a lane, a short last block
                                           ((2, 64, 197), (0,)),  # odd inner: one column to a lane, 788 slots past the workgroup's 64
                                           ((1, 32, 5), (0,)),
                                           ((2, 40, 8), (1,)),    # inner % 4 == 0 from a base one float off: one column to a lane
                                           ((2, 170, 68), (0,))]) # four columns to a lane in tiles of 4 K-blocks x 16 column groups: 6 and 17
def test_cols_path(dev, shape, offsets):
    _check(_data(shape, 100000 * shape[0] + 1000 * shape[1] + shape[2]), 1, dev, shape, offsets)


# ------------------------------------------------------------------------------------------------ 3. special values
def _special_rows():
    """[8, 64]: block 0 of every row is special, block 1 ordinary."""
    ordinary = np.linspace(-3, 3, 32).astype(np.float32)
    x = np.tile(ordinary, (8, 2)).astype(np.float32)
    x[0, 7] = np.nan                                       # a NaN block
    x.view(np.uint32)[0, 9] = 0xFFC00001
    x[1, 9] = np.inf                                       # an inf block
    x[2, 11] = -np.inf
    x[3, :32] = 0
    x[3, 1:32:2] = -0.0                                    # all zero, -0 among them
    x[4, :32] = np.float32(2.0 ** -131)
    x[4, 0] = -np.float32(2.0 ** -130)                     # the maximum is an fp32 subnormal: se = -127
    x[5, :32] = np.float32(2.0 ** -127)
    x[5, 3] = np.float32(2.0 ** -120)                      # subnormal values under se = -127 (E4M3)
    x[6, :32] = np.float32(1.0)
    x[6, 31] = np.float32(3.4028234663852886e38)           # the largest se
    x[7, :32] = np.float32(-3.4028234663852886e38)
    return x


def test_special_values(dev):
    x = _special_rows()
    for elem in ELEMS:
        c, s = P.encode(x, 1, elem)
        assert s[:3, 0].tolist() == [0xFF] * 3 and s[3:5, 0].tolist() == [0, 0] and s[6, 0] == s[7, 0] == 127 - M.EMAX[elem] + 127
        assert s[5, 0] == (0 if elem == "mxfp8" else 5)
        assert (c[:3, :32 if elem == "mxfp8" else 16] == (0x7F if elem == "mxfp8" else 0)).all()
        assert set(np.unique(c[3, :32 if elem == "mxfp8" else 16]).tolist()) == ({0x00, 0x80} if elem == "mxfp8" else {0x80})
    _check(x, 1, dev, "rows", offsets=(0, 1))
    _check(np.ascontiguousarray(x.T), 0, dev, "columns", offsets=(0, 1))      # the same blocks strided: four columns to a lane, then one


# ------------------------------------------------------------------------------------------------ 4. decode on every pair
@pytest.mark.parametrize("elem", ELEMS)
def test_decode_on_every_code_and_scale_pair(dev, elem):
    from dipoorlet_amd import ops
    c, s = P.all_pairs(elem)
    nb = s.size
    want = P.decode(c, s, elem, (nb, 32), 1)
    assert np.isinf(want).any() and np.isnan(want).any()
    dc, ds = torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev)
    got = ops.mx_decode(dc, ds, elem, (nb, 32), 1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))           # (NaN is 0x7FC00000 on both sides)
    # the same bytes are the K-innermost form of the transposed tensor: the strided kernel, four columns to a lane
    got_t = ops.mx_decode(dc, ds.reshape(nb), elem, (32, nb), 0).cpu().numpy()
    assert np.array_equal(got_t.view(np.uint32), np.ascontiguousarray(want.T).view(np.uint32))
    odd = nb - 1                                                                # ... and one column to a lane
    got_o = ops.mx_decode(dc[:odd].contiguous(), ds[:odd].contiguous().reshape(odd), elem, (32, odd), 0).cpu().numpy()
    assert np.array_equal(got_o.view(np.uint32), np.ascontiguousarray(want[:odd].T).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. entry points
def test_entry_points(dev):
    import dipoorlet_amd.torch_ops  # noqa: F401
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    xh = _data((3, 40, 6), 3)
    x = torch.from_numpy(xh).to(dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for elem in ELEMS:
        for axis in (0, 1, 2, -1, -2, -3):
            want_c, want_s = P.encode(xh, axis, elem)
            codes, scales = ops.mx_encode(x, axis, elem)
            assert np.array_equal(codes.cpu().numpy(), want_c) and np.array_equal(scales.cpu().numpy(), want_s), (elem, axis)
            tc, ts = torch.ops.dipoorlet.mx_encode(x, axis, elem)
            assert torch.equal(tc, codes) and torch.equal(ts, scales), ("torch op", elem, axis)
            y = ops.mx_decode(codes, scales, elem, x.shape, axis)
            _same(y.cpu().numpy(), M.fake_quant_mx(xh, axis, elem), (elem, axis))
            ty = torch.ops.dipoorlet.mx_decode(codes, scales, elem, list(x.shape), axis)
            assert torch.equal(ty.view(torch.int32), y.view(torch.int32)), ("torch op", elem, axis)
    xt = x.transpose(0, 2)              # (the torch op makes its input contiguous, as its siblings do)
    tc, ts = torch.ops.dipoorlet.mx_encode(xt, 1, "mxfp4")
    want_c, want_s = P.encode(xt.contiguous().cpu().numpy(), 1, "mxfp4")
    assert np.array_equal(tc.cpu().numpy(), want_c) and np.array_equal(ts.cpu().numpy(), want_s)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fc, fs = torch.ops.dipoorlet.mx_encode(torch.empty(5, 49, 3, device="cuda"), 1, "mxfp4")
        assert tuple(fc.shape) == (5, 3, 32) and tuple(fs.shape) == (5, 3, 2) and fc.dtype == fs.dtype == torch.uint8
        fy = torch.ops.dipoorlet.mx_decode(fc, fs, "mxfp4", [5, 49, 3], 1)
        assert tuple(fy.shape) == (5, 49, 3) and fy.dtype == torch.float32
    # the Python checks
    codes, scales = ops.mx_encode(x, 1, "mxfp8")
    assert tuple(codes.shape) == (3, 6, 64) and tuple(scales.shape) == (3, 6, 2)
    e = ops.mx_encode(torch.empty(0, 5, device=dev), 1, "mxfp8")
    assert tuple(e[0].shape) == (0, 32) and tuple(e[1].shape) == (0, 1)
    assert ops.mx_decode(e[0], e[1], "mxfp8", (0, 5), 1).shape == (0, 5)
    for bad in (dict(elem="mxfp6"), dict(axis=3), dict(axis=-4), dict(axis=None)):
        kw = dict(axis=1, elem="mxfp8")
        kw.update(bad)
        with pytest.raises(_hip.DipoorletHipError):
            ops.mx_encode(x, kw["axis"], kw["elem"])
        with pytest.raises(_hip.DipoorletHipError):
            ops.mx_decode(codes, scales, kw["elem"], x.shape, kw["axis"])
    with pytest.raises(_hip.DipoorletHipError):
        ops.mx_encode(x.transpose(0, 1), 1, "mxfp8")                                       # not contiguous: no silent copy
    with pytest.raises(_hip.DipoorletHipError):
        ops.mx_encode(x.cpu(), 1, "mxfp8")                                                 # no CPU path
    with pytest.raises(_hip.DipoorletHipError):
        ops.mx_decode(codes.cpu(), scales, "mxfp8", x.shape, 1)
    with pytest.raises(_hip.DipoorletHipError, match=r"\[3, 6, 64\]"):
        ops.mx_decode(codes[:, :, :32].contiguous(), scales, "mxfp8", x.shape, 1)          # the unpadded length is not the layout
    with pytest.raises(_hip.DipoorletHipError):
        ops.mx_decode(codes, scales.to(torch.int32), "mxfp8", x.shape, 1)
    with pytest.raises(_hip.DipoorletHipError):
        ops.mx_decode(codes, scales, "mxfp8", x.shape, 1, out=torch.empty(3, 40, 5, device=dev))
    # the C ABI
    buf = torch.full((3 * 6 * 64 + 32,), 0xA5, dtype=torch.uint8, device=dev)
    y = torch.full((3 * 40 * 6,), -77.0, dtype=torch.float32, device=dev)
    px, py, pc, ps = (C.c_void_p(t.data_ptr()) for t in (x, y, buf, scales))
    assert lib.dpl_mx_encode(2, px, 3, 40, 6, pc, ps, st) == -2 and b"elem" in lib.dpl_last_error()
    assert lib.dpl_mx_encode(0, None, 3, 40, 6, pc, ps, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_encode(0, px, 3, 40, 6, None, ps, st) == -2
    assert lib.dpl_mx_encode(0, px, 3, 40, 6, pc, None, st) == -2
    assert lib.dpl_mx_decode(0, pc, None, 3, 40, 6, py, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_encode(0, px, 1, 1 << 31, 1, pc, ps, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_mx_decode(0, pc, ps, 1, 1, 1 << 31, py, st) == -2
    assert lib.dpl_mx_encode(0, px, 1 << 40, 1 << 20, 1 << 20, pc, ps, st) == -2 and b"too large" in lib.dpl_last_error()
    assert lib.dpl_mx_decode(1, pc, ps, 1 << 58, 1, 1, py, st) == -2 and b"too large" in lib.dpl_last_error()     # (32 pad codes per row)
    for zero in ((0, 40, 6), (3, 0, 6), (3, 40, 0)):       # n == 0: a no-op, whatever the pointers
        assert lib.dpl_mx_encode(1, None, *zero, None, None, st) == 0
        assert lib.dpl_mx_decode(1, None, None, *zero, None, st) == 0
    # d_codes off a 16-byte boundary: refused with the message, nothing launched (neither output is touched)
    for shift in (1, 4, 8):
        mis = C.c_void_p(buf.data_ptr() + shift)
        assert lib.dpl_mx_encode(0, px, 3, 40, 6, mis, ps, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
        assert lib.dpl_mx_decode(0, mis, ps, 3, 40, 6, py, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
    torch.cuda.synchronize()
    assert (buf == 0xA5).all() and (y == -77.0).all() and torch.equal(scales, ops.mx_encode(x, 1, "mxfp8")[1])
    # ... and on one it writes the codes and nothing behind them
    assert lib.dpl_mx_encode(0, px, 3, 40, 6, C.c_void_p(buf.data_ptr() + 16), ps, st) == 0
    torch.cuda.synchronize()
    hb = buf.cpu().numpy()
    assert (hb[:16] == 0xA5).all() and (hb[16 + 3 * 6 * 64:] == 0xA5).all() and np.array_equal(hb[16:16 + 3 * 6 * 64], codes.cpu().numpy().reshape(-1))
