"""GPU: the block-scaled product of `--mx_verify` (k_mx_gemm; dpl_mx_gemm, ops.mx_gemm, ops.mx_matmul) against the numpy definition
(tests/mx_gemm_model.py).  The instruction's lane map is not taken on trust: test 1 writes every operand byte by hand so that every
output is ONE product — a wrong k order inside a fragment, a swapped row and column, a block paired with the wrong scale byte or a
wrong nibble order each change some output — and asks for bit equality.  Test 2 draws data whose every partial sum is exact in fp32
in any order (elements 0, +-1, +-2, +-3, +-4, +-6, scale bytes 125 .. 129: every product a multiple of 2^-4 below 36 * 2^4, every
partial sum up to K = 544 below 2^24 such units) and asks for equal values at the shapes where the kernel masks rows, columns and
K-blocks or walks more than one tile or K step.  Only test 4 (random data through the encoder) has a tolerance: Kp * 2^-23 * S for mxfp4, and for mxfp8 — whose products the
instruction truncates inside runs of 8 k before it adds them — twice the worst ratio to that figure measured on the MI355X."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import mx_gemm_model as G

pytestmark = pytest.mark.gpu

ELEMS = ("mxfp8", "mxfp4")
PAIRS = [(a, b) for a in ELEMS for b in ELEMS]
GUARD = 64           # floats around C
SENTINEL = -777.0
EXACT_VALUES = np.array([0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6], np.float64)
SHAPES = [(1, 1, 1), (16, 16, 32), (17, 10, 33), (33, 40, 96), (5, 17, 129), (32, 32, 160), (19, 35, 544)]
ODD = [(17, 10, 33), (33, 40, 96), (5, 17, 129), (19, 35, 544)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _bytes_of(k, elem):
    kp = 32 * -(-k // 32)
    return kp // 2 if elem == "mxfp4" else kp


def _exact_operand(rng, lead, rows, k, elem):
    """Codes and scales of [*lead, rows, Kp] exact-class data; the elements past k are pad: code 0."""
    kp = 32 * -(-k // 32)
    v = rng.choice(EXACT_VALUES, size=tuple(lead) + (rows, kp))
    v[..., k:] = 0.0
    return G.codes_from_values(v, elem), rng.integers(125, 130, size=tuple(lead) + (rows, kp // 32)).astype(np.uint8)


def _run(dev, ac, a_s, bc, b_s, elem_a, elem_b):
    """ops.mx_gemm into a C with a guard band on both sides -> the result on the host (the band is checked)."""
    from dipoorlet_amd import ops
    shape = tuple(ac.shape[:-1]) + (bc.shape[-2],)
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    out = buf[GUARD:GUARD + numel].view(shape)
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (ac, a_s, bc, b_s)]
    assert ops.mx_gemm(*t, elem_a, elem_b, out=out) is out
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + numel:] == SENTINEL).all(), "the guard band around C was written"
    return host[GUARD:GUARD + numel].reshape(shape)


def _same_values(got, want, what):
    """Equal as values (a zero's sign is free), NaN in the same places."""
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~wn & (got != want)))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), [float(got[tuple(i)]) for i in bad[:5]], [float(want[tuple(i)]) for i in bad[:5]])


# ------------------------------------------------------------------------------------------------ 1. the lane map, exact
# row i of A has ONE element, at k = KPOS[i]: all four K-blocks of the 128-wide step, in-block positions 0 .. 31 of both parities
KPOS = [0, 33, 66, 99, 5, 38, 71, 104, 31, 62, 95, 127, 16, 49, 82, 115]
NONZERO = np.array([0.5, 1, 1.5, 2, 3, 4, 6])


def _lane_map_case():
    a, b = np.zeros((16, 128)), np.zeros((16, 128))
    for i, kk in enumerate(KPOS):
        a[i, kk] = NONZERO[(2 * i + 1) % 7] * (-1 if i % 3 == 1 else 1)
    j, kk = np.meshgrid(np.arange(16), np.arange(128), indexing="ij")
    b[:] = NONZERO[(5 * j + 3 * kk + (kk >> 5)) % 7] * np.where((j + kk // 3) % 2 == 1, -1.0, 1.0)       # depends on j AND on kk
    i4, blk = np.meshgrid(np.arange(16), np.arange(4), indexing="ij")
    a_s = (120 + (3 * i4 + 5 * blk) % 13).astype(np.uint8)                                                    # differ per (row, block)
    b_s = (121 + (5 * i4 + 3 * blk) % 11).astype(np.uint8)
    return a, a_s, b, b_s


@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_lane_map_is_exact(dev, elem_a, elem_b):
    a, a_s, b, b_s = _lane_map_case()
    assert sorted({k // 32 for k in KPOS}) == [0, 1, 2, 3] and {k % 2 for k in KPOS} == {0, 1} and len({k % 32 for k in KPOS}) >= 8
    ac, bc = G.codes_from_values(a, elem_a), G.codes_from_values(b, elem_b)
    want, _ = G.mx_gemm(ac, a_s, bc, b_s, elem_a, elem_b)
    # every output is one product: a[i, k_i] 2^(sa - 127) * b[j, k_i] 2^(sb - 127), exact in fp32
    one = np.array([[a[i, KPOS[i]] * b[j, KPOS[i]] * 2.0 ** (int(a_s[i, KPOS[i] // 32]) + int(b_s[j, KPOS[i] // 32]) - 254) for j in range(16)]
                    for i in range(16)])
    assert np.array_equal(want.astype(np.float64), one) and (want != want.T).any() and (want != 0).all()
    got = _run(dev, ac, a_s, bc, b_s, elem_a, elem_b)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:8].tolist(), got[tuple(bad[:8].T)].tolist(), want[tuple(bad[:8].T)].tolist())


# ------------------------------------------------------------------------------------------------ 2. the exact class
@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_exact_class_at_every_masking_shape(dev, elem_a, elem_b):
    rng = np.random.default_rng(len(elem_a) * 7 + len(elem_b))
    shapes = SHAPES if elem_a == elem_b else ODD
    for m, n, k in shapes:
        for lead, b_lead in (((), ()), ((3,), ()), ((3,), (3,))):
            ac, a_s = _exact_operand(rng, lead, m, k, elem_a)
            bc, b_s = _exact_operand(rng, b_lead, n, k, elem_b)
            assert ac.shape[-1] == _bytes_of(k, elem_a)
            want, _ = G.mx_gemm(ac, a_s, bc, b_s, elem_a, elem_b)
            got = _run(dev, ac, a_s, bc, b_s, elem_a, elem_b)
            _same_values(got, want, (m, n, k, lead, b_lead))


def test_two_leading_dimensions_and_the_torch_op(dev):
    import dipoorlet_amd.torch_ops  # noqa: F401
    rng = np.random.default_rng(9)
    ac, a_s = _exact_operand(rng, (2, 3), 17, 40, "mxfp8")
    bc, b_s = _exact_operand(rng, (2, 3), 9, 40, "mxfp4")
    want, _ = G.mx_gemm(ac, a_s, bc, b_s, "mxfp8", "mxfp4")
    _same_values(_run(dev, ac, a_s, bc, b_s, "mxfp8", "mxfp4"), want, "[2, 3] batches")
    t = [torch.from_numpy(x).to(dev) for x in (ac, a_s, bc, b_s)]
    _same_values(torch.ops.dipoorlet.mx_gemm(*t, "mxfp8", "mxfp4").cpu().numpy(), want, "torch.ops")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.ops.dipoorlet.mx_gemm(torch.empty(2, 3, 17, 64, dtype=torch.uint8, device="cuda"), torch.empty(2, 3, 17, 2, dtype=torch.uint8, device="cuda"),
                                        torch.empty(9, 32, dtype=torch.uint8, device="cuda"), torch.empty(9, 2, dtype=torch.uint8, device="cuda"),
                                        "mxfp8", "mxfp4")
        assert tuple(f.shape) == (2, 3, 17, 9) and f.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 3. zero blocks
@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_zero_blocks_contribute_nothing(dev, elem_a, elem_b):
    """What the encoder writes for an all-zero block: scale byte 0, codes 0."""
    rng = np.random.default_rng(17)
    m, n, k = 19, 21, 160
    ac, a_s = _exact_operand(rng, (), m, k, elem_a)
    bc, b_s = _exact_operand(rng, (), n, k, elem_b)
    za, zs = ac.copy(), a_s.copy()
    per = ac.shape[-1] // a_s.shape[-1]
    for r, blk in ((0, 0), (3, 4), (7, 1), (7, 2), (18, 3)):
        za[r, blk * per:(blk + 1) * per], zs[r, blk] = 0, 0
    for r in (5, 16):
        za[r], zs[r] = 0, 0                                               # whole rows
    want, _ = G.mx_gemm(za, zs, bc, b_s, elem_a, elem_b)
    assert (want[5] == 0).all() and (want[0] != 0).any()
    _same_values(_run(dev, za, zs, bc, b_s, elem_a, elem_b), want, "zero blocks in A")
    got = _run(dev, bc, b_s, za, zs, elem_b, elem_a)                      # ... and on the B side
    _same_values(got, want.T, "zero blocks in B")
    # an operand of nothing but such blocks: zeros, no NaN
    for a_side in (True, False):
        z = (np.zeros_like(ac), np.zeros_like(a_s))
        got = _run(dev, *z, bc, b_s, elem_a, elem_b) if a_side else _run(dev, bc, b_s, *z, elem_b, elem_a)
        assert not np.isnan(got).any() and (got == 0).all()
    got = _run(dev, np.zeros_like(ac), np.zeros_like(a_s), np.zeros_like(bc), np.zeros_like(b_s), elem_a, elem_b)
    assert not np.isnan(got).any() and (got == 0).all()


# ------------------------------------------------------------------------------------------------ 4. through the encoder
# |got - ref| <= factor * Kp * 2^-23 * S + 2^-149 (mx_gemm_model.bound).  factor 1 — exact products, fp32 additions in any order —
# holds for mxfp4 (measured ratio: 0).  For mxfp8 it does NOT hold on the MI355X: measured 11.12 and 19.51 on the two shapes below,
# because the instruction truncates the E4M3 products of every run of 8 consecutive k to 2^-14 of the run's largest one before it
# adds them (mx_gemm_model's docstring).  So mxfp8 is held to twice the worst measured ratio: 2 * 19.51.
BOUND_FACTOR = {"mxfp4": 1.0, "mxfp8": G.HW_FACTOR}


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("xs,ws", [((34, 96), (96, 24)), ((2, 17, 64), (64, 48))])
def test_random_data_through_the_encoder(dev, elem, xs, ws):
    from dipoorlet_amd import ops
    rng = np.random.default_rng(xs[0] * 100 + ws[1])
    x, w = rng.standard_normal(xs).astype(np.float32), rng.standard_normal(ws).astype(np.float32)
    x[..., 5] *= 40.0                                                     # a few large channels
    x[..., ws[0] - 3] *= 90.0
    w[7] *= 25.0
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    w_codes, w_scales = ops.mx_encode(wd, 0, elem)
    assert tuple(w_codes.shape) == (ws[1], _bytes_of(ws[0], elem))
    got = ops.mx_matmul(xd, w_codes, w_scales, elem).cpu().numpy()
    assert got.shape == xs[:-1] + (ws[1],)
    x_codes, x_scales = ops.mx_encode(xd, -1, elem)
    ref, s = G.mx_gemm(x_codes.cpu().numpy(), x_scales.cpu().numpy(), w_codes.cpu().numpy(), w_scales.cpu().numpy(), elem)
    kp = 32 * -(-ws[0] // 32)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ratio = float((err / (kp * 2.0 ** -23 * s + 2.0 ** -149)).max())
    print(f"mx_gemm through the encoder {elem} {xs} x {ws}: max |got - ref| / (Kp 2^-23 S) = {ratio:.4g}")
    assert not np.isnan(got).any() and (err <= G.bound(s, kp, BOUND_FACTOR[elem])).all(), ratio
    # and it is the product the fake-quantised graph computes, to that bound
    want = torch.matmul(ops.fake_quant_mx(xd, -1, elem).double(), ops.fake_quant_mx(wd, 0, elem).double()).cpu().numpy()
    assert (np.abs(got - want) <= G.bound(s, kp, BOUND_FACTOR[elem])).all()


# ------------------------------------------------------------------------------------------------ 5. the NaN rule
@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_nan_rule(dev, elem_a, elem_b):
    rng = np.random.default_rng(23)
    m, n, k = 20, 18, 160                                                  # two K steps, the second with one block
    ac, a_s = _exact_operand(rng, (), m, k, elem_a)
    bc, b_s = _exact_operand(rng, (), n, k, elem_b)
    for blk in (0, 2, 4):
        s1 = a_s.copy()
        s1[3, blk] = 0xFF
        got = _run(dev, ac, s1, bc, b_s, elem_a, elem_b)
        assert np.isnan(got[3]).all() and np.isfinite(np.delete(got, 3, axis=0)).all(), blk
        _same_values(got, G.mx_gemm(ac, s1, bc, b_s, elem_a, elem_b)[0], ("A scale", blk))
        s2 = b_s.copy()
        s2[11, blk] = 0xFF
        got = _run(dev, ac, a_s, bc, s2, elem_a, elem_b)
        assert np.isnan(got[:, 11]).all() and np.isfinite(np.delete(got, 11, axis=1)).all(), blk
        _same_values(got, G.mx_gemm(ac, a_s, bc, s2, elem_a, elem_b)[0], ("B scale", blk))
    if elem_a == "mxfp8":
        for code, at in ((0x7F, 1), (0xFF, 70), (0x7F, 159)):
            c1 = ac.copy()
            c1[3, at] = code
            z = bc.copy()
            z[:, at // 2 if elem_b == "mxfp4" else at] = 0                 # against zeros of B at that k: still NaN
            got = _run(dev, c1, a_s, z, b_s, elem_a, elem_b)
            assert np.isnan(got[3]).all() and np.isfinite(np.delete(got, 3, axis=0)).all(), (code, at)
    if elem_b == "mxfp8":
        c1 = bc.copy()
        c1[17, 133] = 0x7F
        got = _run(dev, ac, a_s, c1, b_s, elem_a, elem_b)
        assert np.isnan(got[:, 17]).all() and np.isfinite(np.delete(got, 17, axis=1)).all()
        _same_values(got, G.mx_gemm(ac, a_s, c1, b_s, elem_a, elem_b)[0], "B code")


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(dev):
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    rng = np.random.default_rng(5)
    ac, a_s = _exact_operand(rng, (), 8, 64, "mxfp8")
    bc, b_s = _exact_operand(rng, (), 6, 64, "mxfp8")
    a, sa, b, sb = (torch.from_numpy(x).to(dev) for x in (ac, a_s, bc, b_s))
    out = torch.full((8, 6), SENTINEL, dtype=torch.float32, device=dev)
    for args, pat in (((a, sa, b, sb, "mxfp6"), r"'mxfp8' or 'mxfp4'"), ((a, sa, b, sb, "mxfp8", "e5m2"), r"'mxfp8' or 'mxfp4'"),
                      ((a, sa, b[:, :32].contiguous(), sb, "mxfp8"), r"B must be codes"),                 # 32 codes against 2 scale bytes
                      ((a, sa, b[:, :32].contiguous(), sb[:, :1].contiguous(), "mxfp8"), r"same number of K-blocks"),
                      ((a, sa, b, sb, "mxfp4"), r"must be codes"),                                        # fp8 bytes are not Kp / 2 nibble pairs
                      ((a[None], sa[None], torch.stack([b, b]), torch.stack([sb, sb]), "mxfp8"), r"leading dimensions"),
                      ((a, sa[:7].contiguous(), b, sb, "mxfp8"), r"A must be codes"),
                      ((a.cpu(), sa, b, sb, "mxfp8"), r"no CPU path"), ((a, sa.int(), b, sb, "mxfp8"), r"uint8"),
                      ((a[0], sa[0], b, sb, "mxfp8"), r"A must be codes")):
        with pytest.raises(_hip.DipoorletHipError, match=pat):
            ops.mx_gemm(*args, out=out) if len(args) == 6 else ops.mx_gemm(*args, None, out)
    with pytest.raises(_hip.DipoorletHipError, match=r"out must have shape \[8, 6\]"):
        ops.mx_gemm(a, sa, b, sb, "mxfp8", out=torch.empty(6, 8, device=dev))
    with pytest.raises(_hip.DipoorletHipError, match=r"at least two dimensions"):
        ops.mx_matmul(torch.zeros(64, device=dev), b, sb, "mxfp8")
    # the C ABI
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    big = torch.zeros(8 * 64 + 32, dtype=torch.uint8, device=dev)
    pa, psa, pb, psb, pc, pbig = (C.c_void_p(t.data_ptr()) for t in (a, sa, b, sb, out, big))
    assert lib.dpl_mx_gemm(2, 0, pa, psa, pb, psb, 1, 8, 6, 64, 0, pc, st) == -2 and b"elem" in lib.dpl_last_error()
    assert lib.dpl_mx_gemm(0, -1, pa, psa, pb, psb, 1, 8, 6, 64, 0, pc, st) == -2 and b"elem" in lib.dpl_last_error()
    assert lib.dpl_mx_gemm(0, 0, None, psa, pb, psb, 1, 8, 6, 64, 0, pc, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_gemm(0, 0, pa, psa, pb, psb, 1, 8, 6, 64, 0, None, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_mx_gemm(0, 0, pa, psa, pb, psb, 1, 1 << 31, 6, 64, 0, pc, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_mx_gemm(0, 0, pa, psa, pb, psb, 1, 8, 6, 1 << 31, 0, pc, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_mx_gemm(0, 0, pa, psa, pb, psb, 1 << 40, 1 << 20, 6, 1 << 20, 0, pc, st) == -2 and b"too large" in lib.dpl_last_error()
    assert lib.dpl_mx_gemm(0, 0, pa, psa, pb, psb, 1 << 30, 1 << 10, 1 << 10, 32, 0, pc, st) == -2 and b"too large" in lib.dpl_last_error()   # the grid
    for zero in ((0, 8, 6, 64), (1, 0, 6, 64), (1, 8, 0, 64), (1, 8, 6, 0)):
        assert lib.dpl_mx_gemm(1, 1, None, None, None, None, *zero, 0, None, st) == 0
    for shift in (1, 4, 8):
        mis = C.c_void_p(big.data_ptr() + shift)
        assert lib.dpl_mx_gemm(0, 0, mis, psa, pb, psb, 1, 8, 6, 64, 0, pc, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
        assert lib.dpl_mx_gemm(0, 0, pa, psa, mis, psb, 1, 6, 8, 64, 0, pc, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call launched"
    assert lib.dpl_mx_gemm(0, 0, pbig, psa, pb, psb, 1, 8, 6, 64, 0, pc, st) == 0          # and on a boundary it runs
    torch.cuda.synchronize()
    assert (out == 0).all()
