"""GPU: the Q/DQ pair, its given-scale form and the scale search for the two MXFP6 formats (k_fake_quant_mx_*, k_mx_scale_search_*
instantiated for Fmt<DPL_MX_E2M3> / Fmt<DPL_MX_E3M2>) against tests/mx_fp6_model.py, bit for bit, scale bytes included: both walks,
both vector widths (a base one float off takes the element-wise kernels), short last blocks, NaN / inf / zero blocks, every code
and tie under several shared exponents, se = -127."""
import gc

import numpy as np
import pytest
import torch

import mx_fp6_model as F
from test_mx_gpu import GUARD, _data, _same, _special_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _run(x, axis, elem, dev, misaligned=False, given=None):
    """ops.fake_quant_mx (given: ops.fake_quant_mx_scaled under those bytes) on a copy of x whose base is 16-byte aligned, or one
    float off -> (y, scales written or None); the floats and the scale bytes around the outputs must come back untouched."""
    from dipoorlet_amd import ops
    off = 1 if misaligned else 0
    n = x.size
    nsc = (n // x.shape[axis]) * -(-x.shape[axis] // 32)
    bx = torch.zeros(n + 2 * GUARD + off, dtype=torch.float32, device=dev)
    by = torch.full((n + 2 * GUARD + off,), -77.0, dtype=torch.float32, device=dev)
    bs = torch.full((nsc + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    xv, yv = bx[GUARD + off:GUARD + off + n].view(x.shape), by[GUARD + off:GUARD + off + n].view(x.shape)
    assert xv.data_ptr() % 16 == 4 * off and yv.data_ptr() % 16 == 4 * off
    xv.copy_(torch.from_numpy(x))
    if given is None:
        ret = ops.fake_quant_mx(xv, axis, elem, out=yv, scales=bs[GUARD:GUARD + nsc])
    else:
        ret = ops.fake_quant_mx_scaled(xv, axis, elem, torch.from_numpy(given).to(dev), out=yv)
    assert ret is yv
    hy, hs = by.cpu().numpy(), bs.cpu().numpy()
    assert (hy[:GUARD + off] == -77.0).all() and (hy[GUARD + off + n:] == -77.0).all(), "written outside y"
    assert (hs[:GUARD] == 0xA5).all() and (hs[GUARD + nsc:] == 0xA5).all(), "written outside scales"
    return hy[GUARD + off:GUARD + off + n].reshape(x.shape), (hs[GUARD:GUARD + nsc] if given is None else None)


def _block_shape(shape, axis):
    """x's shape with the block axis replaced by its number of blocks: the shape of the scale bytes in x's own order."""
    axis %= len(shape)
    return tuple(shape[:axis]) + (-(-shape[axis] // 32),) + tuple(shape[axis + 1:])


def _given_bytes(rng, floor, elem):
    """Bytes around the floor rule's: the floor, one up, one down, 0xFF, and one above the format's limit."""
    g = floor.astype(np.int64) + rng.integers(-1, 2, floor.shape)
    g = np.clip(np.where(floor == 0xFF, 100, g), 0, 254)
    flat = g.reshape(-1)
    flat[::7] = 0xFF
    flat[3::11] = 255 - F.EMAX[elem]
    return g.astype(np.uint8)


def _check(x, axis, dev, what, misaligned=(False, True)):
    rng = np.random.default_rng(x.size)
    for elem in F.ELEMS:
        want_y, want_s = F.fake_quant_mx(x, axis, elem, return_scales=True)
        given = _given_bytes(rng, want_s, elem).reshape(_block_shape(x.shape, axis))
        want_g = F.fake_quant_mx_scaled(x, axis, elem, given)
        for mis in misaligned:
            y, s = _run(x, axis, elem, dev, mis)
            _same(y, want_y, (what, elem, mis))
            assert np.array_equal(s, want_s.reshape(-1)), (what, elem, mis, np.flatnonzero(s != want_s.reshape(-1))[:5])
            y, _ = _run(x, axis, elem, dev, mis, given=given)
            _same(y, want_g, (what, elem, mis, "given"))
            y, _ = _run(x, axis, elem, dev, mis, given=want_s.reshape(given.shape))        # the floor's own bytes: the plain pair
            _same(y, want_y, (what, elem, mis, "given the floor"))


# ------------------------------------------------------------------------------------------------ 1. contiguous blocks
@pytest.mark.parametrize("K", [1, 31, 32, 33, 127, 128, 129])
def test_contiguous_path(dev, K):
    for rows in (1, 67):                                                    # 67 rows of 5 blocks: more than one workgroup's 32 / 128 groups
        _check(_data((rows, K), 1000 * rows + K), 1, dev, (rows, K))


# ------------------------------------------------------------------------------------------------ 2. strided blocks
@pytest.mark.parametrize("inner", [1, 3, 4, 68])
@pytest.mark.parametrize("K", [32, 33, 96])
def test_strided_path(dev, K, inner):
    _check(_data((2, K, inner), 1000 * K + inner), 1, dev, (2, K, inner))


# ------------------------------------------------------------------------------------------------ 3. rounding
@pytest.mark.parametrize("elem", F.ELEMS)
def test_every_code_tie_and_neighbour(dev, elem):
    """boundary_points(elem) * 2^se, 31 to a block beside a sentinel (the format's largest value times 2^se) that pins the block's
    shared exponent to se — -127, where inputs and outputs are fp32 subnormals, and the largest one the format allows."""
    pts = F.boundary_points(elem)
    nb = -(-pts.size // 31)
    top_se = 127 - F.EMAX[elem]
    blocks = []
    for se in (-127, -20, 0, 30, top_se):
        blk = np.zeros((nb, 32), np.float64)
        blk[:, 0] = F.ELEM_MAX[elem]
        blk[:, 1:].reshape(-1)[:pts.size] = pts
        blocks.append(np.ldexp(blk, se).astype(np.float32))
    x = np.concatenate(blocks)
    want_y, want_s = F.fake_quant_mx(x, 1, elem, return_scales=True)
    assert sorted(set(want_s.reshape(-1).tolist())) == [0, 107, 127, 157, top_se + 127]
    for xx, axis, wy, ws in ((x, 1, want_y, want_s.reshape(-1)), (np.ascontiguousarray(x.T), 0, want_y.T, want_s[:, 0, 0])):
        for mis in (False, True):
            y, s = _run(xx, axis, elem, dev, mis)
            _same(y, wy, (elem, axis, mis))
            assert np.array_equal(s, ws), (elem, axis, mis)


# ------------------------------------------------------------------------------------------------ 4. special values
def test_special_values(dev):
    x = _special_rows()
    for elem in F.ELEMS:
        want, s = F.fake_quant_mx(x, 1, elem, return_scales=True)
        assert np.isnan(want[1:4, :32]).all() and s[0, 0, 0] == 0 and s[4, 0, 0] == 0 and s[10, 0, 0] == 0 and (s[1:4, 0, 0] == 0xFF).all()
    _check(x, 1, dev, "rows")
    _check(np.ascontiguousarray(x.T), 0, dev, "columns")
    _check(np.ascontiguousarray(x[:11].T), 0, dev, "columns, 11")


# ------------------------------------------------------------------------------------------------ 5. the scale search
def _search_data(shape, seed, elem):
    x = _data(shape, seed)
    x3 = x.reshape(shape[0], shape[1], -1)
    x3[0, :min(32, shape[1])] = 0                                              # a lone value just under the end of its binade: se0 + 1 wins
    x3[0, min(5, shape[1] - 1)] = np.float32(0.999 * 2.0 ** (F.EMAX[elem] + 1))
    if shape[1] > 40:
        x3[-1, 40] = np.inf
    return x


@pytest.mark.parametrize("elem", F.ELEMS)
@pytest.mark.parametrize("shape", [(5, 1), (5, 33), (67, 128), (3, 129), (2, 32, 3), (2, 33, 4), (2, 96, 68)])
def test_scale_search_bytes_and_errors(dev, elem, shape):
    from dipoorlet_amd import ops
    x = _search_data(shape, 17 * len(shape) + shape[1], elem)
    want_s, want_e = F.scale_search(x, 1, elem)
    floor = F.fake_quant_mx(x, 1, elem, return_scales=True)[1]
    moved = (want_s != floor)
    assert moved.any() and (~moved).any()                                      # both choices occur
    for mis in (False, True):
        off = 1 if mis else 0
        buf = torch.zeros(x.size + 4 + off, dtype=torch.float32, device=dev)
        xv = buf[4 + off:4 + off + x.size].view(x.shape)
        xv.copy_(torch.from_numpy(x))
        assert xv.data_ptr() % 16 == 4 * off
        err = torch.full(_block_shape(x.shape, 1) + (2,), -1.0, dtype=torch.float64, device=dev)
        got = ops.mx_scale_search(xv, 1, elem, err=err)
        assert np.array_equal(got.cpu().numpy().reshape(want_s.shape), want_s), (elem, shape, mis)
        assert np.array_equal(err.cpu().numpy().reshape(want_e.shape).view(np.uint64), want_e.view(np.uint64)), (elem, shape, mis)


def test_refusals_launch_nothing(dev):
    import ctypes as C

    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    x = torch.ones(4, 64, device=dev)
    y = torch.full((4, 64), -77.0, device=dev)
    for bad in ("mxfp6", "e5m2", "mxfp6_e2m1"):
        with pytest.raises(_hip.DipoorletHipError, match=r"'mxfp8' or 'mxfp4' \(or 'mxfp6_e2m3' / 'mxfp6_e3m2'\)"):
            ops.fake_quant_mx(x, 1, bad, out=y)
        with pytest.raises(_hip.DipoorletHipError, match=r"'mxfp8' or 'mxfp4'"):
            ops.mx_scale_search(x, 1, bad)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc = torch.full((8,), 0xA5, dtype=torch.uint8, device=dev)
    px, py, ps = (C.c_void_p(t.data_ptr()) for t in (x, y, sc))
    for code in (2, 3, 4, 5, 8, -1):
        assert lib.dpl_fake_quant_mx(code, px, py, 4, 64, 1, ps, st) == -2 and b"DPL_MX_E2M3 / DPL_MX_E3M2" in lib.dpl_last_error()
        assert lib.dpl_fake_quant_mx_scaled(code, px, py, 4, 64, 1, ps, st) == -2 and b"elem must be DPL_MX_E4M3 or DPL_MX_E2M1" in lib.dpl_last_error()
        assert lib.dpl_mx_scale_search(code, px, 4, 64, 1, ps, None, st) == -2
    w = torch.ones(4, 64, device=dev)
    u = torch.eye(64, device=dev)
    for elem in F.ELEMS:
        with pytest.raises(_hip.DipoorletHipError, match=r"gptq_mx_block: elem must be 'mxfp8' or 'mxfp4' \(the recursion"):
            ops.gptq_mx_block(w, 0, 32, u, elem)
    err = torch.zeros(4, 32, device=dev)
    for code in (6, 7):
        rc = lib.dpl_gptq_mx_block(code, C.c_void_p(w.data_ptr()), 4, 64, 64, 0, 32, C.c_void_p(u.data_ptr()), 64, C.c_void_p(err.data_ptr()), ps, 2, st)
        assert rc == -2 and b"elem must be DPL_MX_E4M3 or DPL_MX_E2M1" in lib.dpl_last_error()
    torch.cuda.synchronize()
    assert (y == -77.0).all() and (sc == 0xA5).all() and (w == 1).all(), "a refused call launched"
