"""GPU: ops.gptq_hessian (dpl_gptq_hessian: H += X^T X as an fp64 SYRK, X dense or the patches of a convolution gathered in the
kernel) against plain numpy in fp64: pad, gather the windows with a strided loop, X^T X.

Two data sets per case.  Integers in [-15, 15]: every product and every sum is exact, so H equals the reference bit for bit — a
wrong gather index, tile mirror or row split has no tolerance to hide in.  N(0, 1): products of fp32 values are exact in fp64, so
only the fp64 additions err, at most rows of them per element on either side: |H - ref| <= 2 rows 2^-53 (|X|^T |X|)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (x shape, kernel, strides, pads [top, left, bottom, right], dilations); a 2-D shape: the dense form, (rows, K)
CASES = [((1, 1),), ((33, 64),), ((70, 65),), ((257, 200),), ((4096, 64),),
         ((2, 3, 9, 8), (3, 3), (1, 1), (1, 1, 1, 1), (1, 1)),          # K = 27
         ((1, 5, 11, 7), (3, 2), (2, 1), (0, 1, 2, 0), (1, 2)),         # K = 30: asymmetric pads, stride and dilation differ per axis
         ((2, 16, 6, 6), (1, 1), (2, 2), (0, 0, 0, 0), (1, 1)),         # K = 16
         ((1, 8, 12, 12), (3, 3), (1, 1), (0, 0, 0, 0), (1, 1)),        # K = 72: crosses a tile edge
         ((3, 64, 5, 5), (1, 1), (1, 1), (0, 0, 0, 0), (1, 1))]         # K = 64 exactly, 75 rows
IDS = ["x".join(map(str, c[0])) + ("" if len(c) == 1 else "-k" + "x".join(map(str, c[1]))) for c in CASES]


def _rows(x, kernel=None, strides=None, pads=None, dil=None):
    """X [rows, K] of the reference: x itself, or its convolution patches in (C, kh, kw) order."""
    if kernel is None:
        return x
    (kh, kw), (sy, sx), (pt, pl, pb, pr), (dy, dx) = kernel, strides, pads, dil
    xp = np.pad(x, ((0, 0), (0, 0), (pt, pb), (pl, pr)))
    oh, ow = (xp.shape[2] - dy * (kh - 1) - 1) // sy + 1, (xp.shape[3] - dx * (kw - 1) - 1) // sx + 1
    cols = np.empty((x.shape[0], oh, ow, x.shape[1], kh, kw), x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, :, ky * dy:ky * dy + (oh - 1) * sy + 1:sy, kx * dx:kx * dx + (ow - 1) * sx + 1:sx]
            cols[:, :, :, :, ky, kx] = win.transpose(0, 2, 3, 1)
    return cols.reshape(x.shape[0] * oh * ow, -1)


def _data(shape, kind):
    rng = np.random.default_rng(sum(shape) + len(kind))
    return (rng.integers(-15, 16, shape) if kind == "int" else rng.standard_normal(shape)).astype(np.float32)


def _device(x, case, H):
    from dipoorlet_amd import ops
    xd = torch.from_numpy(x).cuda()
    if len(case) == 1:
        return ops.gptq_hessian(xd, H)
    return ops.gptq_hessian(xd, H, weight_shape=(7, x.shape[1]) + case[1], strides=case[2], pads=case[3], dilations=case[4])


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hessian_against_fp64_numpy(case, kind):
    from dipoorlet_amd import ops
    x = _data(case[0], kind)
    X = _rows(x, *case[1:]).astype(np.float64)
    rows, K = X.shape
    if case[0] == (4096, 64):
        assert ops.gptq_hessian_splits(rows, K) >= 4           # the smallest case on the partial-tile path
    H = torch.zeros((K, K), dtype=torch.float64, device="cuda")
    assert _device(x, case, H) == rows
    got, ref = H.cpu().numpy(), X.T @ X
    if kind == "int":
        assert np.array_equal(got, ref)
    else:
        excess = np.abs(got - ref) - 2 * rows * 2.0 ** -53 * (np.abs(X).T @ np.abs(X))
        print(f"{case[0]}: max |H - ref| {np.abs(got - ref).max():.3e}, largest excess over the bound {excess.max():.3e}")
        assert (excess <= 0).all()
    assert np.array_equal(got, got.T)


def test_two_calls_accumulate_and_repeat_bit_for_bit():
    """(4096, 64), integers: the halves added by two calls (each split in ranges, the second onto what the first left) are the
    whole, exactly; H is symmetric; the same call on a zeroed H twice gives the same bits."""
    from dipoorlet_amd import ops
    x = _data((4096, 64), "int")
    xd = torch.from_numpy(x).cuda()
    H = torch.zeros((64, 64), dtype=torch.float64, device="cuda")
    assert ops.gptq_hessian(xd[:2048], H) + ops.gptq_hessian(xd[2048:], H) == 4096
    X = x.astype(np.float64)
    assert np.array_equal(H.cpu().numpy(), X.T @ X) and torch.equal(H, H.t())
    xn = torch.from_numpy(_data((4096, 64), "normal")).cuda()
    twice = [torch.zeros((64, 64), dtype=torch.float64, device="cuda") for _ in range(2)]
    for h in twice:
        ops.gptq_hessian(xn, h)
    assert torch.equal(twice[0], twice[1]) and torch.equal(twice[0], twice[0].t())


@pytest.mark.parametrize("what,reason", [("cpu", "no CPU path"), ("fp16", "contiguous float32"), ("fp32_h", "float64"),
                                         ("k", "K mismatch"), ("extent", "output extent")])
def test_refusals(what, reason):
    from dipoorlet_amd import _hip, ops
    x = torch.zeros((2, 3, 4, 4), device="cpu" if what == "cpu" else "cuda", dtype=torch.float16 if what == "fp16" else torch.float32)
    H = torch.zeros((28, 28) if what == "k" else (27, 27), dtype=torch.float32 if what == "fp32_h" else torch.float64, device="cuda")
    weight_shape = (8, 3, 7, 3) if what == "extent" else (8, 3, 3, 3)
    if what == "extent":
        H = torch.zeros((63, 63), dtype=torch.float64, device="cuda")
    with pytest.raises(_hip.DipoorletHipError, match=reason):
        ops.gptq_hessian(x, H, weight_shape=weight_shape, pads=(1, 1, 1, 1))
