"""GPU: ops.mx_conv (k_mx_conv) with MXFP6 operands on the exact class — elements 0, +-1, +-2, +-3, +-4, +-6 and scale bytes
125 .. 129, whose every partial sum is exact in fp32 in any order — for FP6 x FP6 of both formats and one mixed pair.  The tap
addressing is tests/test_mx_conv_gpu.py's subject and the lane map tests/test_mx_fp6_gemm_gpu.py's; what is new here is the 24-byte
block behind a pixel: C = 3 (one short block), 32, 33 (a second, short block) and 64, where an odd number of channel blocks a pixel
puts every other pixel's codes 8 bytes off a 16-byte boundary."""
import gc

import numpy as np
import pytest
import torch

import mx_fp6_model as F
from test_mx_conv_gpu import EXACT_VALUES, _geometry, _run, _same_values
from test_mx_fp6_gemm_gpu import codes_from_values

pytestmark = pytest.mark.gpu

PAIRS = [("mxfp6_e2m3", "mxfp6_e2m3"), ("mxfp6_e3m2", "mxfp6_e3m2"), ("mxfp6_e3m2", "mxfp4")]
GEOMETRIES = [(3, (2, 2), (1, 1)), (1, (1, 1), (0, 0))]              # (kernel, strides, pads): 3 x 3 pad 1 stride 2, and 1 x 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _exact_operand(rng, lead, c, elem):
    cp = 32 * -(-c // 32)
    v = rng.choice(EXACT_VALUES, size=tuple(lead) + (cp,))
    v[..., c:] = 0.0
    return codes_from_values(v, elem), rng.integers(125, 130, size=tuple(lead) + (cp // 32,)).astype(np.uint8)


def conv_ref(ac, a_s, bc, b_s, elem_a, elem_b, strides, pads, dilations, out_hw):
    """tests/mx_conv_model.py's sum over the decoded bytes, in fp64: C[b, oy, ox, co] = sum over ky, kx, ch of
    a[b, oy sh - pt + ky dh, ox sw - pl + kx dw, ch] * b[co, ky, kx, ch], a tap outside the image contributing nothing."""
    a, b = F.decoded64(ac, a_s, elem_a), F.decoded64(bc, b_s, elem_b)
    n, h, w, _ = a.shape
    cout, kh, kw, _ = b.shape
    out = np.zeros((n,) + tuple(out_hw) + (cout,))
    for ky in range(kh):
        for kx in range(kw):
            for oy in range(out_hw[0]):
                for ox in range(out_hw[1]):
                    iy, ix = oy * strides[0] - pads[0] + ky * dilations[0], ox * strides[1] - pads[1] + kx * dilations[1]
                    if 0 <= iy < h and 0 <= ix < w:
                        out[:, oy, ox, :] += a[:, iy, ix, :] @ b[:, ky, kx, :].T
    return out


@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
@pytest.mark.parametrize("c", [3, 32, 33, 64])
def test_exact_class(dev, elem_a, elem_b, c):
    rng = np.random.default_rng(100 * c + len(elem_a) + len(elem_b))
    n, h, w, cout = 2, 9, 9, 5
    for k, strides, pads in GEOMETRIES:
        ac, a_s = _exact_operand(rng, (n, h, w), c, elem_a)
        bc, b_s = _exact_operand(rng, (cout, k, k), c, elem_b)
        assert ac.shape[-1] == F.BYTES_PER_BLOCK[elem_a] * -(-c // 32)
        geo = _geometry(h, w, k, k, strides, pads, (1, 1))
        assert geo["out_hw"] == ((5, 5) if k == 3 else (9, 9))
        want = conv_ref(ac, a_s, bc, b_s, elem_a, elem_b, **geo)
        assert np.abs(want).max() < 2.0 ** 24 * 2.0 ** -4 and (want != 0).any()          # every partial sum is exact in fp32
        _same_values(_run(dev, ac, a_s, bc, b_s, elem_a, elem_b, geo), want.astype(np.float32), (c, k))
    # the 0xFF rule: a bad pixel makes the outputs its taps reach NaN and leaves the others finite; a bad weight block its channel
    k, strides, pads = GEOMETRIES[0]
    geo = _geometry(h, w, k, k, strides, pads, (1, 1))
    ac, a_s = _exact_operand(rng, (n, h, w), c, elem_a)
    bc, b_s = _exact_operand(rng, (cout, k, k), c, elem_b)
    s1 = a_s.copy()
    s1[1, 4, 4, -1] = 0xFF
    got = _run(dev, ac, s1, bc, b_s, elem_a, elem_b, geo)
    reached = np.zeros((n, 5, 5), bool)
    for oy in range(5):
        for ox in range(5):
            reached[1, oy, ox] = abs(2 * oy - 4) <= 1 and abs(2 * ox - 4) <= 1
    assert np.isnan(got[reached]).all() and np.isfinite(got[~reached]).all() and reached.sum() == 1
    s2 = b_s.copy()
    s2[3, 2, 0, 0] = 0xFF
    got = _run(dev, ac, a_s, bc, s2, elem_a, elem_b, geo)
    assert np.isnan(got[..., 3]).all() and np.isfinite(np.delete(got, 3, axis=-1)).all()


def test_refusals(dev):
    from dipoorlet_amd import _hip, ops
    rng = np.random.default_rng(1)
    ac, a_s = _exact_operand(rng, (1, 4, 4), 33, "mxfp6_e2m3")
    bc, b_s = _exact_operand(rng, (2, 1, 1), 33, "mxfp6_e2m3")
    t = [torch.from_numpy(x).to(dev) for x in (ac, a_s, bc, b_s)]
    kw = dict(strides=(1, 1), pads=(0, 0), dilations=(1, 1), out_hw=(4, 4))
    with pytest.raises(_hip.DipoorletHipError, match=r"'mxfp8' or 'mxfp4' \(or 'mxfp6_e2m3' / 'mxfp6_e3m2'\)"):
        ops.mx_conv(*t, "mxfp6", **kw)
    with pytest.raises(_hip.DipoorletHipError, match=r"A must be codes \[n, h, w, Cp\]"):
        ops.mx_conv(*t, "mxfp8", "mxfp6_e2m3", **kw)
    got = ops.mx_conv(*t, "mxfp6_e2m3", **kw).cpu().numpy()
    _same_values(got, conv_ref(ac, a_s, bc, b_s, "mxfp6_e2m3", "mxfp6_e2m3", **kw).astype(np.float32), "1 x 1")
