"""GPU: k_mx_smooth_err (dpl_mx_smooth_err, ops.mx_smooth_err), no tolerance anywhere: exact data against tests/mx_smooth_model.py,
general data (NaN and inf included, twice) against the composed path, and refusals that launch nothing."""
import functools

import numpy as np
import pytest
import torch

import mx_smooth_model as S
from dipoorlet_amd.weight_transform.smooth import smooth_scales

pytestmark = pytest.mark.gpu

ELEMS = ("mxfp8", "mxfp4")
VALUES = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -.5, -1, -1.5, -2, -3, -4, -6], np.float32)       # values of E2M1, and of E4M3
# (m, n, k, n_cand): every m of {1, 63, 65}, n of {1, 64, 70}, k of {1, 31, 32, 33, 127, 128, 129, 300}, n_cand of {1, 3}
EXACT = [(1, 1, 1, 1), (63, 64, 31, 3), (65, 70, 32, 1), (1, 70, 33, 3), (65, 1, 127, 1), (63, 64, 128, 3), (65, 64, 129, 1), (63, 70, 300, 3)]


dev = pytest.fixture(scope="module")(lambda: torch.device("cuda:0"))


def _same_bits(got, want, what):
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~wn & (got.view(np.uint64) != want.view(np.uint64))))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


def _run(dev, x, w, s, ref, elem, offset=0):
    """-> (sums [n_cand, 2], part) on the host; offset: floats by which x, w and s sit off a 16-byte boundary."""
    from dipoorlet_amd import ops
    def put(v):
        view = torch.empty(v.size + 4, dtype=torch.float32, device=dev)[offset:offset + v.size].view(v.shape)
        return view.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    part = torch.full((s.shape[0], -(-x.shape[0] // 64), -(-w.shape[0] // 64), 2), -777.0, dtype=torch.float64, device=dev)
    sums = ops.mx_smooth_err(put(x), put(w), put(s), torch.from_numpy(ref).to(dev), elem, part=part)
    return sums.cpu().numpy(), part.cpu().numpy()


# Values of the format times a power of two per block, s a power of two per block: every quotient and product is exact, Q/DQ is the
# identity, and a product of two elements is a multiple of 2^-2 below 2^8, so over kp <= 320 every fp32 partial sum is exact (< 2^17).
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "x".join(str(v) for v in s))
def test_exact_data_equals_the_model(dev, elem, shape):
    m, n, k, n_cand = shape
    rng = np.random.default_rng(sum(shape))
    nblk = -(-k // 32)
    def per_block(rows, choices):
        return np.repeat(rng.choice(np.array(choices, np.float32), size=(rows, nblk)), 32, axis=1)[:, :k]
    x = rng.choice(VALUES, size=(m, k)) * per_block(m, (1, 2))
    w = rng.choice(VALUES, size=(n, k)) * per_block(n, (1, 2))
    s = per_block(n_cand, (1, 2))
    ref = rng.standard_normal((m, n)).astype(np.float32) * 8
    want = S.smooth_err_partials(x, w, s, ref, elem)
    sums, part = _run(dev, x, w, s, ref, elem)
    _same_bits(part, want, shape)
    _same_bits(sums, functools.reduce(np.add, want.reshape(n_cand, -1, 2).transpose(1, 0, 2), np.zeros((n_cand, 2))), "ascending tiles")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape,special,offset", [((65, 70, 160), False, 0), ((65, 70, 160), False, 1), ((130, 64, 257), False, 1),
                                                  ((65, 70, 160), True, 0)],
                         ids=["65x70x160", "65x70x160-off-16-bytes", "130x64x257-scalar", "65x70x160-nan-inf"])
def test_general_data_equals_the_composed_path(dev, elem, shape, special, offset):
    from dipoorlet_amd import ops
    m, n, k = shape
    rng = np.random.default_rng(m + k)
    x = rng.standard_normal((m, k)).astype(np.float32)
    x[:, [3, 40, k - 1]] *= 50.0
    w = (0.05 * rng.standard_normal((n, k))).astype(np.float32)
    s = np.stack([smooth_scales(np.abs(x).max(0), np.abs(w).max(0), a) for a in (0.25, 0.5, 0.75)])
    if special:
        x[2, 40] = np.nan                                                # row 2 of C, every candidate
        s[1, 100] = np.inf                                               # w * inf: every column of candidate 1
    xd, wd, sd = (torch.from_numpy(v).to(dev) for v in (x, w, s))
    ref = torch.matmul(torch.nan_to_num(xd), wd.t()).contiguous()
    want = torch.stack([ops.mx_gemm_err(*ops.mx_encode(xd / sd[c], -1, elem), *ops.mx_encode(wd * sd[c], -1, elem), ref, elem)
                        for c in range(3)]).cpu().numpy()
    assert np.isnan(want[..., 0]).any() == special and not np.isnan(want[0, 1:, :, 0]).any()
    runs = [_run(dev, x, w, s, ref.cpu().numpy(), elem, offset=offset) for _ in range(2)]
    _same_bits(runs[0][1], want, shape)
    _same_bits(runs[1][1], runs[0][1], "second run")
    _same_bits(runs[1][0], runs[0][0], "second run's sums")


@pytest.mark.parametrize("case,rc,words", [("fp6", -2, "elem must be DPL_MX_E4M3 or DPL_MX_E2M1"), ("no_cand", 0, ""),
                                           ("cand_65", -2, "n_cand must be in [1, 64]"), ("null_x", -2, "must not be null")])
def test_refusals_launch_nothing(dev, case, rc, words):
    from dipoorlet_amd import _hip
    lib = _hip.lib()
    m, n, k = 8, 8, 32
    x, w, ref = (torch.ones(r, c, device=dev) for r, c in ((m, k), (n, k), (m, n)))
    s = torch.ones(65, k, device=dev)
    part = torch.full((65, 2), -777.0, dtype=torch.float64, device=dev)
    elem = 6 if case == "fp6" else _hip.MX_E2M1
    n_cand = {"no_cand": 0, "cand_65": 65}.get(case, 2)
    px = None if case == "null_x" else x.data_ptr()
    got = lib.dpl_mx_smooth_err(elem, px, w.data_ptr(), s.data_ptr(), n_cand, m, n, k, ref.data_ptr(), part.data_ptr(), None)
    torch.cuda.synchronize()
    assert got == rc and (rc == 0 or words in lib.dpl_last_error().decode()) and bool((part == -777.0).all())
    with pytest.raises(ValueError):
        __import__("dipoorlet_amd.ops").ops.mx_smooth_err(x, w, s, ref, "mxfp4")      # 65 candidates
