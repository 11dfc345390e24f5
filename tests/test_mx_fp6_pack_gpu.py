"""GPU: the packed form of the two MXFP6 formats (k_mx_encode_*, k_mx_decode_* on the 24-byte block; dpl_mx_encode,
dpl_mx_encode_scaled, dpl_mx_decode) against tests/mx_fp6_model.py, byte for byte: a block is at a multiple of 8 bytes, not of 16,
and the code array of an odd number of blocks ends 8 bytes short of a 16-byte boundary — so every array the kernels write sits
inside a band of 0xA5 bytes that must come back untouched, at block counts 1, 2, 3 and 5, on both walks and both vector widths."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import mx_fp6_model as F
from test_mx_pack_gpu import _data, _placed, _same, _special_rows

pytestmark = pytest.mark.gpu
GUARD = 64           # bytes around every array a kernel writes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _banded(nbytes, dev):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + nbytes]


def _band_ok(buf, nbytes):
    h = buf.cpu().numpy()
    return (h[:GUARD] == 0xA5).all() and (h[GUARD + nbytes:] == 0xA5).all()


def _split(shape, axis):
    axis %= len(shape)
    return int(np.prod(shape[:axis], dtype=np.int64)), int(shape[axis]), int(np.prod(shape[axis + 1:], dtype=np.int64))


def _encode(xv, axis, elem, dev, given=None):
    """dpl_mx_encode (given: dpl_mx_encode_scaled) into banded arrays -> (codes, scales) as device tensors; the bands are checked."""
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    cs, ss = F.packed_shapes(tuple(xv.shape), axis, elem)
    nc, ns = int(np.prod(cs)), int(np.prod(ss))
    outer, k, inner = _split(tuple(xv.shape), axis)
    cbuf, codes = _banded(nc, dev)
    sbuf, scales = _banded(ns, dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px, pc, ps = (C.c_void_p(t.data_ptr()) for t in (xv, codes, scales))
    if given is None:
        rc = lib.dpl_mx_encode(ops.MX_ELEM[elem], px, outer, k, inner, pc, ps, st)
    else:
        rc = lib.dpl_mx_encode_scaled(ops.MX_ELEM[elem], px, outer, k, inner, C.c_void_p(given.data_ptr()), pc, ps, st)
    assert rc == 0, lib.dpl_last_error()
    torch.cuda.synchronize()
    assert _band_ok(cbuf, nc), "written outside the codes"
    assert _band_ok(sbuf, ns), "written outside the scales"
    return codes.view(cs), scales.view(ss)


def _check(x, axis, dev, what, offsets=(0, 1)):
    """Every claim of this file on one tensor, per format and per base offset of the fp32 side (one float off: VEC = 1)."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(x.size)
    for elem in F.ELEMS:
        want_c, want_s = F.encode(x, axis, elem)
        want_y, qdq_s = F.fake_quant_mx(x, axis, elem, return_scales=True)
        nblk = want_s.shape[-1]
        assert want_c.shape[-1] == 24 * nblk
        given = np.clip(qdq_s.astype(np.int64) + rng.integers(0, 2, qdq_s.shape), 0, 254).astype(np.uint8)
        given.reshape(-1)[::5] = 0xFF
        want_gc, want_gs = F.encode_scaled(x, axis, elem, given)
        for off in offsets:
            xv = _placed(x, dev, off)
            codes, scales = _encode(xv, axis, elem, dev)
            hc, hs = codes.cpu().numpy(), scales.cpu().numpy()
            assert np.array_equal(hs, want_s), (what, elem, off, "scales")
            assert np.array_equal(hc, want_c), (what, elem, off, "codes", np.flatnonzero(hc != want_c)[:5])
            oc, os_ = ops.mx_encode(xv, axis, elem)                             # the Python entry: the same bytes, the model's shapes
            assert tuple(oc.shape) == want_c.shape and torch.equal(oc, codes) and torch.equal(os_, scales)
            # the scale bytes are the Q/DQ kernel's, K-innermost
            sc = torch.empty(qdq_s.shape, dtype=torch.uint8, device=dev)
            y_qdq = ops.fake_quant_mx(xv, axis, elem, scales=sc)
            assert np.array_equal(sc.cpu().numpy().transpose(0, 2, 1).reshape(-1), hs.reshape(-1)), (what, elem, off, "axis swap")
            # decode into a banded buffer at the same offset
            n = x.size
            by = torch.full((n + 2 * (GUARD // 4) + off,), -77.0, dtype=torch.float32, device=dev)
            yv = by[GUARD // 4 + off:GUARD // 4 + off + n].view(x.shape)
            assert ops.mx_decode(codes.contiguous(), scales.contiguous(), elem, x.shape, axis, out=yv) is yv
            hy = by.cpu().numpy()
            assert (hy[:GUARD // 4 + off] == -77.0).all() and (hy[GUARD // 4 + off + n:] == -77.0).all(), (what, elem, off, "written outside y")
            got = hy[GUARD // 4 + off:GUARD // 4 + off + n]
            _same(got, y_qdq.cpu().numpy(), (what, elem, off, "decode(encode) vs fake_quant_mx"))
            _same(got, want_y, (what, elem, off, "decode(encode) vs model"))
            # under given bytes
            gd = torch.from_numpy(given.reshape(-1)).to(dev)
            gc_, gs_ = _encode(xv, axis, elem, dev, given=gd)
            assert np.array_equal(gs_.cpu().numpy(), want_gs) and np.array_equal(gc_.cpu().numpy(), want_gc), (what, elem, off, "given")


# ------------------------------------------------------------------------------------------------ 1. contiguous blocks
@pytest.mark.parametrize("K", [32, 64, 96, 160, 1, 31, 33, 130])                # 1, 2, 3 and 5 blocks; short last blocks (VEC = 1: K % 4 != 0)
def test_rows_path(dev, K):
    for rows in (1, 3, 67):                                                     # odd block counts in all: the array ends off a 16-byte boundary
        _check(_data((rows, K), 1000 * rows + K), 1, dev, (rows, K))


# ------------------------------------------------------------------------------------------------ 2. strided blocks
@pytest.mark.parametrize("inner", [3, 4, 68])
@pytest.mark.parametrize("K", [32, 33, 96, 160])
def test_cols_path(dev, K, inner):
    _check(_data((1, K, inner), 1000 * K + inner), 1, dev, (1, K, inner))
    if K == 96:
        _check(_data((3, K, inner), K + inner), 1, dev, (3, K, inner))


# ------------------------------------------------------------------------------------------------ 3. special values
def test_special_values(dev):
    x = _special_rows()
    for elem in F.ELEMS:
        c, s = F.encode(x, 1, elem)
        assert s[:3, 0].tolist() == [0xFF] * 3 and s[3:5, 0].tolist() == [0, 0] and s[6, 0] == s[7, 0] == 127 - F.EMAX[elem] + 127
        assert (c[:3, :24] == 0).all()                                          # a 0xFF block: every code 0
        assert set(np.unique(F.unpack6(c[3, :24])).tolist()) == {0x00, 0x20}    # zeros of both signs
    _check(x, 1, dev, "rows")
    _check(np.ascontiguousarray(x.T), 0, dev, "columns")
    pts = np.concatenate([F.boundary_points(e) for e in F.ELEMS])
    pts = np.concatenate([pts, np.zeros(-pts.size % 32, np.float32)]).reshape(-1, 32)
    _check(pts, 1, dev, "boundary points")
    _check(np.ascontiguousarray((pts * np.float32(2.0 ** -126)).T), 0, dev, "boundary points near se = -127, strided")


# ------------------------------------------------------------------------------------------------ 4. decode on every pair
@pytest.mark.parametrize("elem", F.ELEMS)
def test_decode_on_every_code_and_scale_byte(dev, elem):
    """The full product: all 64 codes — as four blocks, 0 .. 31, 63 .. 32, 32 .. 63 and 31 .. 0, so that every code sits at two bit
    positions — under each of the scale bytes 0, 1, 127, 254 - emax and 0xFF: 20 blocks, block 5 * set + byte.  Under 0xFF every code,
    the negative ones included, is the one NaN pattern 0x7FC00000.  Laid out as rows of one block (and 19 of them: the code array
    then ends 8 bytes short of a 16-byte boundary), as one row of 20 blocks, and strided with four columns and one column to a lane."""
    from dipoorlet_amd import ops
    bytes_ = np.array([0, 1, 127, 254 - F.EMAX[elem], 0xFF], np.uint8)
    sets = np.stack([np.arange(32), np.arange(63, 31, -1), np.arange(32, 64), np.arange(31, -1, -1)]).astype(np.uint8)
    codes6 = np.repeat(sets, 5, axis=0)                                          # [20, 32]
    s = np.tile(bytes_, 4)
    assert {(int(cc), int(b)) for row, b in zip(codes6, s) for cc in row} == {(cc, int(b)) for cc in range(64) for b in bytes_}
    c = F.pack6(codes6)                                                          # [20, 24]
    want = F.decode_elements(codes6, s[:, None], elem)                           # [20, 32]
    nan = s == 0xFF
    assert nan.sum() == 4 and (want[nan].view(np.uint32) == 0x7FC00000).all() and np.isfinite(want[~nan]).all()
    for shape, axis, cc, ss, ww in (((20, 32), 1, c, s.reshape(20, 1), want),                                    # rows, 16-byte vectors
                                    ((19, 32), 1, c[1:], s[1:].reshape(19, 1), want[1:]),                        # an odd number of blocks
                                    ((1, 640), 1, c.reshape(1, -1), s.reshape(1, 20), want.reshape(1, -1)),      # 20 blocks a row
                                    ((32, 20), 0, c, s, np.ascontiguousarray(want.T)),                           # strided, four columns to a lane
                                    ((32, 19), 0, c[1:], s[1:], np.ascontiguousarray(want[1:].T))):              # strided, one
        for off in (0, 1):
            n = int(np.prod(shape))
            by = torch.full((n + 32 + off,), -77.0, dtype=torch.float32, device=dev)
            yv = by[16 + off:16 + off + n].view(shape)
            ops.mx_decode(torch.from_numpy(np.ascontiguousarray(cc)).to(dev), torch.from_numpy(np.ascontiguousarray(ss)).to(dev), elem, shape, axis, out=yv)
            hy = by.cpu().numpy()
            assert (hy[:16 + off] == -77.0).all() and (hy[16 + off + n:] == -77.0).all()
            assert np.array_equal(hy[16 + off:16 + off + n].view(np.uint32), ww.reshape(-1).view(np.uint32)), (shape, off)


# ------------------------------------------------------------------------------------------------ 5. entry points
def test_torch_ops_and_refusals(dev):
    import dipoorlet_amd.torch_ops  # noqa: F401
    from dipoorlet_amd import _hip, ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    lib = _hip.lib()
    x = torch.from_numpy(_data((3, 70, 4), 3)).to(dev)
    for elem in F.ELEMS:
        c, s = torch.ops.dipoorlet.mx_encode(x, 1, elem)
        wc, ws = F.encode(x.cpu().numpy(), 1, elem)
        assert np.array_equal(c.cpu().numpy(), wc) and np.array_equal(s.cpu().numpy(), ws) and tuple(c.shape) == (3, 4, 72)
        y = torch.ops.dipoorlet.mx_decode(c, s, elem, [3, 70, 4], 1)
        _same(y.cpu().numpy(), F.fake_quant_mx(x.cpu().numpy(), 1, elem), elem)
        _same(torch.ops.dipoorlet.fake_quant_mx(x, 1, elem).cpu().numpy(), y.cpu().numpy(), elem)
        with FakeTensorMode():
            fc, fs = torch.ops.dipoorlet.mx_encode(torch.empty(3, 70, 4, device="cuda"), 1, elem)
            assert tuple(fc.shape) == (3, 4, 72) and tuple(fs.shape) == (3, 4, 3) and fc.dtype == torch.uint8
        with pytest.raises(_hip.DipoorletHipError, match=r"has codes \[3, 4, 72\]"):
            ops.mx_decode(c[..., :64].contiguous(), s, elem, (3, 70, 4), 1)
    # refusals launch nothing
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cbuf, codes = _banded(3 * 4 * 72, dev)
    sbuf, scales = _banded(36, dev)
    y = torch.full((3, 70, 4), -77.0, device=dev)
    px, pc, ps, py = (C.c_void_p(t.data_ptr()) for t in (x, codes, scales, y))
    for code in (2, 5, 8):
        assert lib.dpl_mx_encode(code, px, 3, 70, 4, pc, ps, st) == -2 and b"DPL_MX_E2M3 / DPL_MX_E3M2" in lib.dpl_last_error()
        assert lib.dpl_mx_decode(code, pc, ps, 3, 70, 4, py, st) == -2 and b"elem must be DPL_MX_E4M3 or DPL_MX_E2M1" in lib.dpl_last_error()
    for shift in (4, 8):                                                        # a block lies at a multiple of 8; the base must not
        mis = C.c_void_p(codes.data_ptr() + shift)
        assert lib.dpl_mx_encode(6, px, 3, 70, 4, mis, ps, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
        assert lib.dpl_mx_decode(7, mis, ps, 3, 70, 4, py, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
    assert lib.dpl_mx_encode(6, None, 3, 70, 4, pc, ps, st) == -2 and b"null" in lib.dpl_last_error()
    torch.cuda.synchronize()
    assert (cbuf == 0xA5).all() and (sbuf == 0xA5).all() and (y == -77.0).all(), "a refused call launched"
