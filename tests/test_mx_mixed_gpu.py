"""GPU: the fused error reduction of `--mx_mixed` (k_mx_gemm_err; dpl_mx_gemm_err, ops.mx_gemm_err) against its definition
(tests/mx_mixed_model.py gemm_err_partials).  Nothing here has a tolerance.  (a) exact operands as tests/test_mx_gemm_gpu.py builds
them — elements 0, +-1 .. +-6 and scale bytes 125 .. 129, every partial sum exact in fp32 in any order — so that the model's C is the
kernel's accumulator, and the partials must equal the model's bit for bit, additions in the defined order included; (b) random data
through the encoder, where the accumulator is only known from ops.mx_gemm's own output: the partials equal the model applied to
that, bit for bit; (c) guard bands around ref and part; (d) the NaN rule; (e) refusals and zero sizes launch nothing."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import mx_gemm_model as G
import mx_mixed_model as X

pytestmark = pytest.mark.gpu

ELEMS = ("mxfp8", "mxfp4")
PAIRS = [(a, b) for a in ELEMS for b in ELEMS]
EXACT_VALUES = np.array([0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6], np.float64)
SHAPES = [(1, 1, 1, 1), (1, 8, 6, 64), (3, 130, 65, 100), (2, 64, 64, 160)]        # (batch, m, n, k)
GUARD = 64
SENTINEL = -777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _exact_operand(rng, lead, rows, k, elem):
    kp = 32 * -(-k // 32)
    v = rng.choice(EXACT_VALUES, size=tuple(lead) + (rows, kp))
    v[..., k:] = 0.0
    return G.codes_from_values(v, elem), rng.integers(125, 130, size=tuple(lead) + (rows, kp // 32)).astype(np.uint8)


def _run(dev, ac, a_s, bc, b_s, ref, elem_a, elem_b, bias):
    """ops.mx_gemm_err with ref and part as views inside sentinel-filled buffers -> part on the host (the bands are checked, and
    that every row of part was written)."""
    from dipoorlet_amd import ops
    m, n = ac.shape[-2], bc.shape[-2]
    shape = tuple(ac.shape[:-2]) + (-(-m // 64), -(-n // 64), 2)
    numel = int(np.prod(shape))
    rbuf = torch.full((ref.size + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    rview = rbuf[GUARD:GUARD + ref.size].view(ref.shape)
    rview.copy_(torch.from_numpy(np.ascontiguousarray(ref)))
    pbuf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    out = pbuf[GUARD:GUARD + numel].view(shape)
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (ac, a_s, bc, b_s)]
    b = None if bias is None else torch.from_numpy(bias).to(dev)
    assert ops.mx_gemm_err(*t, rview, elem_a, elem_b, bias=b, out=out) is out
    torch.cuda.synchronize()
    host, rhost = pbuf.cpu().numpy(), rbuf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + numel:] == SENTINEL).all(), "the guard band around part was written"
    assert (rhost[:GUARD] == SENTINEL).all() and (rhost[GUARD + ref.size:] == SENTINEL).all() and np.array_equal(
        rhost[GUARD:GUARD + ref.size].view(np.uint32), np.ascontiguousarray(ref).reshape(-1).view(np.uint32)), "ref or its guard band was written"
    got = host[GUARD:GUARD + numel].reshape(shape)
    assert (got != SENTINEL).all(), "a row of part was not written"
    return got


def _same_bits(got, want, what):
    """Equal bit for bit; a NaN matches a NaN."""
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~wn & (got.view(np.uint64) != want.view(np.uint64))))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), [float(got[tuple(i)]) for i in bad[:5]], [float(want[tuple(i)]) for i in bad[:5]])


# ------------------------------------------------------------------------------------------------ (a) exact data
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_exact_data_bit_for_bit(dev, shape):
    batch, m, n, k = shape
    rng = np.random.default_rng(batch * 1000 + m + n + k)
    pairs = PAIRS if shape == SHAPES[1] else [(e, e) for e in ELEMS]
    for elem_a, elem_b in pairs:
        for b_lead in ((), (batch,)):                                     # B shared, B batched
            ac, a_s = _exact_operand(rng, (batch,), m, k, elem_a)
            bc, b_s = _exact_operand(rng, b_lead, n, k, elem_b)
            c, _ = G.mx_gemm(ac, a_s, bc, b_s, elem_a, elem_b)
            ref = (c + rng.integers(-3, 4, size=c.shape)).astype(np.float32)      # small integers: d is exact, and differs per element
            bias_v = rng.integers(-2, 3, size=n).astype(np.float32)
            for bias in (None, bias_v):
                want = X.gemm_err_partials(c, ref, bias)
                assert want.shape == (batch, -(-m // 64), -(-n // 64), 2) and (m * n < 48 or (want[..., 0] > 0).any())
                got = _run(dev, ac, a_s, bc, b_s, ref, elem_a, elem_b, bias)
                _same_bits(got, want, (shape, elem_a, elem_b, b_lead, bias is not None))


def test_no_leading_dimension_and_two(dev):
    rng = np.random.default_rng(3)
    for lead in ((), (2, 2)):
        ac, a_s = _exact_operand(rng, lead, 70, 96, "mxfp4")
        bc, b_s = _exact_operand(rng, (), 9, 96, "mxfp4")
        c, _ = G.mx_gemm(ac, a_s, bc, b_s, "mxfp4")
        ref = (c * 0.5).astype(np.float32)
        got = _run(dev, ac, a_s, bc, b_s, ref, "mxfp4", None, None)
        assert got.shape == lead + (2, 1, 2)
        _same_bits(got, X.gemm_err_partials(c, ref), lead)


# ------------------------------------------------------------------------------------------------ (b) random data: the same accumulator
@pytest.mark.parametrize("elem", ELEMS)
def test_random_data_is_mx_gemms_accumulator(dev, elem):
    from dipoorlet_amd import ops
    rng = np.random.default_rng(11 if elem == "mxfp8" else 12)
    batch, m, n, k = 3, 130, 65, 100
    x, w = rng.standard_normal((batch, m, k)).astype(np.float32), rng.standard_normal((k, n)).astype(np.float32)
    x[..., 5] *= 40.0                                                    # a few large channels
    w[7] *= 25.0
    bias = rng.standard_normal(n).astype(np.float32)
    xd, wd, bd = (torch.from_numpy(v).to(dev) for v in (x, w, bias))
    ref = torch.matmul(xd, wd) + bd
    a_codes, a_scales = ops.mx_encode(xd, -1, elem)
    b_codes, b_scales = ops.mx_encode(wd, 0, elem)
    c = ops.mx_gemm(a_codes, a_scales, b_codes, b_scales, elem).cpu().numpy()
    for b in (None, bd):
        got = ops.mx_gemm_err(a_codes, a_scales, b_codes, b_scales, ref, elem, bias=b).cpu().numpy()
        want = X.gemm_err_partials(c, ref.cpu().numpy(), None if b is None else bias)
        _same_bits(got, want, (elem, b is not None))
        # (and it is an error measure: against the plain fp64 sums, to rounding)
        dd, rr = X.gemm_err_terms(c, ref.cpu().numpy(), None if b is None else bias)
        assert np.isclose(got[..., 0].sum(), dd.sum(), rtol=1e-12, atol=0) and np.isclose(got[..., 1].sum(), rr.sum(), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ (d) the NaN rule
@pytest.mark.parametrize("elem", ELEMS)
def test_nan_rule(dev, elem):
    rng = np.random.default_rng(23)
    batch, m, n, k = 2, 130, 65, 160
    ac, a_s = _exact_operand(rng, (batch,), m, k, elem)
    bc, b_s = _exact_operand(rng, (), n, k, elem)
    c, _ = G.mx_gemm(ac, a_s, bc, b_s, elem)
    ref = (c + 1.0).astype(np.float32)
    clean = _run(dev, ac, a_s, bc, b_s, ref, elem, elem, None)
    assert np.isfinite(clean).all()
    s1 = a_s.copy()
    s1[1, 70, 2] = 0xFF                                                   # row 70 of batch 1: tile row 1, both tile columns
    got = _run(dev, ac, s1, bc, b_s, ref, elem, elem, None)
    hit = np.zeros(got.shape[:-1], bool)
    hit[1, 1, :] = True
    assert np.isnan(got[hit][:, 0]).all(), "the tiles that hold the row"
    _same_bits(got[hit][:, 1], clean[hit][:, 1], "the reference's own sum is untouched")
    _same_bits(got[~hit], clean[~hit], "every other tile")
    _same_bits(got, X.gemm_err_partials(G.mx_gemm(ac, s1, bc, b_s, elem)[0], ref), "the model")


# ------------------------------------------------------------------------------------------------ (e) refusals and zero sizes
def test_refusals_launch_nothing(dev):
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    rng = np.random.default_rng(5)
    ac, a_s = _exact_operand(rng, (), 8, 64, "mxfp8")
    bc, b_s = _exact_operand(rng, (), 6, 64, "mxfp8")
    a, sa, b, sb = (torch.from_numpy(x).to(dev) for x in (ac, a_s, bc, b_s))
    ref = torch.zeros((8, 6), dtype=torch.float32, device=dev)
    bias = torch.zeros(6, dtype=torch.float32, device=dev)
    out = torch.full((1, 1, 2), SENTINEL, dtype=torch.float64, device=dev)
    E = _hip.DipoorletHipError
    for args, kw, pat in (((a, sa, b, sb, ref, "mxfp6"), {}, r"'mxfp8' or 'mxfp4'"), ((a, sa, b, sb, ref, "mxfp8", "e5m2"), {}, r"'mxfp8' or 'mxfp4'"),
                          ((a, sa, b[:, :32].contiguous(), sb, ref, "mxfp8"), {}, r"B must be codes"),
                          ((a, sa, b[:, :32].contiguous(), sb[:, :1].contiguous(), ref, "mxfp8"), {}, r"same number of K-blocks"),
                          ((a, sa, b, sb, ref, "mxfp4"), {}, r"must be codes"),
                          ((a[None], sa[None], torch.stack([b, b]), torch.stack([sb, sb]), ref[None], "mxfp8"), {}, r"leading dimensions"),
                          ((a.cpu(), sa, b, sb, ref, "mxfp8"), {}, r"no CPU path"), ((a, sa.int(), b, sb, ref, "mxfp8"), {}, r"uint8"),
                          ((a, sa, b, sb, ref.cpu(), "mxfp8"), {}, r"ref must be a ROCm device tensor"),
                          ((a, sa, b, sb, ref.double(), "mxfp8"), {}, r"ref must be contiguous float32"),
                          ((a, sa, b, sb, ref.t(), "mxfp8"), {}, r"ref must be contiguous float32"),
                          ((a, sa, b, sb, ref[:7].contiguous(), "mxfp8"), {}, r"ref must have shape \[8, 6\]"),
                          ((a, sa, b, sb, ref, "mxfp8"), {"bias": bias[:5].contiguous()}, r"bias must have shape \[6\]"),
                          ((a, sa, b, sb, ref, "mxfp8"), {"bias": bias.double()}, r"bias must be contiguous float32"),
                          ((a, sa, b, sb, ref, "mxfp8"), {"out": torch.empty((1, 1, 2), device=dev)}, r"out must be a contiguous float64"),
                          ((a, sa, b, sb, ref, "mxfp8"), {"out": torch.empty((1, 2), dtype=torch.float64, device=dev)}, r"shape \[1, 1, 2\]")):
        with pytest.raises(E, match=pat):
            ops.mx_gemm_err(*args, **{"out": out, **kw})
    # the C ABI
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    big = torch.zeros(8 * 64 + 32, dtype=torch.uint8, device=dev)
    pa, psa, pb, psb, pr, pbias, pp, pbig = (C.c_void_p(t.data_ptr()) for t in (a, sa, b, sb, ref, bias, out, big))
    f = lib.dpl_mx_gemm_err
    assert f(2, 0, pa, psa, pb, psb, 1, 8, 6, 64, 0, pr, None, pp, st) == -2 and b"elem" in lib.dpl_last_error()
    assert f(0, -1, pa, psa, pb, psb, 1, 8, 6, 64, 0, pr, None, pp, st) == -2 and b"elem" in lib.dpl_last_error()
    assert f(0, 0, None, psa, pb, psb, 1, 8, 6, 64, 0, pr, None, pp, st) == -2 and b"null" in lib.dpl_last_error()
    assert f(0, 0, pa, psa, pb, psb, 1, 8, 6, 64, 0, None, pbias, pp, st) == -2 and b"d_ref" in lib.dpl_last_error()
    assert f(0, 0, pa, psa, pb, psb, 1, 8, 6, 64, 0, pr, pbias, None, st) == -2 and b"d_part" in lib.dpl_last_error()
    assert f(0, 0, pa, psa, pb, psb, 1, 1 << 31, 6, 64, 0, pr, None, pp, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert f(0, 0, pa, psa, pb, psb, 1, 8, 6, 1 << 31, 0, pr, None, pp, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert f(0, 0, pa, psa, pb, psb, 1 << 40, 1 << 20, 6, 1 << 20, 0, pr, None, pp, st) == -2 and b"too large" in lib.dpl_last_error()
    assert f(0, 0, pa, psa, pb, psb, 1 << 30, 1 << 10, 1 << 10, 32, 0, pr, None, pp, st) == -2 and b"too large" in lib.dpl_last_error()   # the grid
    for zero in ((0, 8, 6, 64), (1, 0, 6, 64), (1, 8, 0, 64), (1, 8, 6, 0)):
        assert f(1, 1, None, None, None, None, *zero, 0, None, None, None, st) == 0
    for shift in (1, 4, 8):
        mis = C.c_void_p(big.data_ptr() + shift)
        assert f(0, 0, mis, psa, pb, psb, 1, 8, 6, 64, 0, pr, None, pp, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
        assert f(0, 0, pa, psa, mis, psb, 1, 6, 8, 64, 0, pr, None, pp, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call launched"
    assert f(0, 0, pbig, psa, pb, psb, 1, 8, 6, 64, 0, pr, pbias, pp, st) == 0              # and on a boundary it runs
    torch.cuda.synchronize()
    assert (out == 0).all()
