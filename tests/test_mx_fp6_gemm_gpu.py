"""GPU: the two MXFP6 formats on the block-scaled MFMA (k_mx_gemm over the 12 pairs that hold an FP6 operand; ops.mx_gemm,
ops.mx_matmul) against tests/mx_fp6_model.py.  As tests/test_mx_gemm_gpu.py does for mxfp8 / mxfp4: the lane map with outputs that
are ONE product each (every bit of the 6-bit codes in use, B depending on j and on k: a wrong K-block per lane group, a wrong bit
order inside the six registers or a wrong scale byte changes some output), the exact class at every masking shape, zero blocks, the
0xFF rule, and random data through the encoder under the factor measured per format (mx_verify.BOUND_FACTOR)."""
import gc

import numpy as np
import pytest
import torch

import mx_fp6_model as F
import mx_gemm_model as G
from test_mx_gemm_gpu import EXACT_VALUES, KPOS, ODD, SHAPES, _run, _same_values

pytestmark = pytest.mark.gpu

PAIRS = [(a, b) for a in F.ALL_ELEMS for b in F.ALL_ELEMS if a in F.ELEMS or b in F.ELEMS]
assert len(PAIRS) == 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def codes_from_values(v, elem):
    """[..., Kp] values of the element format -> its packed codes (mx_gemm_model.codes_from_values for the other two formats)."""
    if elem not in F.ELEMS:
        return G.codes_from_values(v, elem)
    v = np.asarray(v, np.float64)
    c = F.codes(elem).astype(np.float64)
    idx = np.minimum(np.searchsorted(c, np.abs(v)), c.size - 1)
    assert np.array_equal(c[idx], np.abs(v)), "not a value of the element format"
    return F.pack6((idx | (np.signbit(v).astype(np.int64) << 5)).astype(np.uint8))


def _ref(ac, a_s, bc, b_s, elem_a, elem_b):
    """(C fp32, S) of the decoded bytes, mx_gemm_model.mx_gemm's for any pair of the four formats."""
    a, b = F.decoded64(ac, a_s, elem_a), F.decoded64(bc, b_s, elem_b)
    bad = np.isnan(a).any(-1)[..., :, None] | np.isnan(b).any(-1)[..., None, :]
    a0, bt = np.nan_to_num(a), np.swapaxes(np.nan_to_num(b), -1, -2)
    return np.where(bad, np.nan, np.matmul(a0, bt)).astype(np.float32), np.where(bad, np.nan, np.matmul(np.abs(a0), np.abs(bt)))


def _exact_operand(rng, lead, rows, k, elem):
    kp = 32 * -(-k // 32)
    v = rng.choice(EXACT_VALUES, size=tuple(lead) + (rows, kp))
    v[..., k:] = 0.0
    return codes_from_values(v, elem), rng.integers(125, 130, size=tuple(lead) + (rows, kp // 32)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. the lane map, exact
def _lane_map_case(elem_a, elem_b):
    """Row i of A has ONE element, at k = KPOS[i]; B depends on j and on k; both draw on every non-zero value of their format, both
    signs, so that every bit of a code is set somewhere at every kind of position; the scale bytes differ per (row, block)."""
    va, vb = F.values_of(elem_a)[1:].astype(np.float64), F.values_of(elem_b)[1:].astype(np.float64)
    if elem_a == "mxfp8":
        va = va[va <= 30]                                                   # (products stay far inside fp32)
    if elem_b == "mxfp8":
        vb = vb[vb <= 30]
    a, b = np.zeros((16, 128)), np.zeros((16, 128))
    for i, kk in enumerate(KPOS):
        a[i, kk] = va[(7 * i + 3) % va.size] * (-1 if i % 3 == 1 else 1)
    j, kk = np.meshgrid(np.arange(16), np.arange(128), indexing="ij")
    b[:] = vb[(5 * j + 3 * kk + (kk >> 5)) % vb.size] * np.where((j + kk // 3) % 2 == 1, -1.0, 1.0)
    i4, blk = np.meshgrid(np.arange(16), np.arange(4), indexing="ij")
    a_s = (120 + (3 * i4 + 5 * blk) % 13).astype(np.uint8)
    b_s = (121 + (5 * i4 + 3 * blk) % 11).astype(np.uint8)
    return a, a_s, b, b_s


@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_lane_map_is_exact(dev, elem_a, elem_b):
    a, a_s, b, b_s = _lane_map_case(elem_a, elem_b)
    ac, bc = codes_from_values(a, elem_a), codes_from_values(b, elem_b)
    want, _ = _ref(ac, a_s, bc, b_s, elem_a, elem_b)
    one = np.array([[a[i, KPOS[i]] * b[j, KPOS[i]] * 2.0 ** (int(a_s[i, KPOS[i] // 32]) + int(b_s[j, KPOS[i] // 32]) - 254) for j in range(16)]
                    for i in range(16)])
    assert np.array_equal(want.astype(np.float64), one) and (want != want.T).any() and (want != 0).all()
    for e, c in ((elem_a, ac), (elem_b, bc)):
        if e in F.ELEMS:                                                    # every bit of the 6-bit codes is set somewhere
            assert np.bitwise_or.reduce(F.unpack6(c).reshape(-1)) == 63
    got = _run(dev, ac, a_s, bc, b_s, elem_a, elem_b)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:8].tolist(), got[tuple(bad[:8].T)].tolist(), want[tuple(bad[:8].T)].tolist())
    got = _run(dev, bc, b_s, ac, a_s, elem_b, elem_a)                       # the one-element operand on the B side
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want.T).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. the exact class
@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_exact_class_at_every_masking_shape(dev, elem_a, elem_b):
    """Elements 0, +-1, +-2, +-3, +-4, +-6 exist in all four formats; with scale bytes 125 .. 129 every partial sum is exact in
    fp32 in any order.  Odd block counts put the last 24-byte block 8 bytes short of a 16-byte boundary."""
    rng = np.random.default_rng(len(elem_a) * 7 + len(elem_b))
    for m, n, k in SHAPES:
        for lead, b_lead in (((), ()), ((3,), ()), ((3,), (3,))):
            ac, a_s = _exact_operand(rng, lead, m, k, elem_a)
            bc, b_s = _exact_operand(rng, b_lead, n, k, elem_b)
            assert ac.shape[-1] == F.BYTES_PER_BLOCK[elem_a] * -(-k // 32)
            want, _ = _ref(ac, a_s, bc, b_s, elem_a, elem_b)
            _same_values(_run(dev, ac, a_s, bc, b_s, elem_a, elem_b), want, (m, n, k, lead, b_lead))
    assert ODD[0] in SHAPES


# ------------------------------------------------------------------------------------------------ 3. zero blocks
@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_zero_blocks_contribute_nothing(dev, elem_a, elem_b):
    rng = np.random.default_rng(17)
    m, n, k = 19, 21, 160
    ac, a_s = _exact_operand(rng, (), m, k, elem_a)
    bc, b_s = _exact_operand(rng, (), n, k, elem_b)
    za, zs = ac.copy(), a_s.copy()
    per = F.BYTES_PER_BLOCK[elem_a]
    for r, blk in ((0, 0), (3, 4), (7, 1), (7, 2), (18, 3)):
        za[r, blk * per:(blk + 1) * per], zs[r, blk] = 0, 0
    for r in (5, 16):
        za[r], zs[r] = 0, 0
    want, _ = _ref(za, zs, bc, b_s, elem_a, elem_b)
    assert (want[5] == 0).all() and (want[0] != 0).any()
    _same_values(_run(dev, za, zs, bc, b_s, elem_a, elem_b), want, "zero blocks in A")
    _same_values(_run(dev, bc, b_s, za, zs, elem_b, elem_a), want.T, "zero blocks in B")
    got = _run(dev, np.zeros_like(ac), np.zeros_like(a_s), np.zeros_like(bc), np.zeros_like(b_s), elem_a, elem_b)
    assert not np.isnan(got).any() and (got == 0).all()


# ------------------------------------------------------------------------------------------------ 4. the 0xFF rule
@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_nan_rule(dev, elem_a, elem_b):
    """For an FP6 operand a 0xFF scale byte is the only source of NaN: every code, 0x3F and the sign bit included, is a number."""
    rng = np.random.default_rng(23)
    m, n, k = 20, 18, 160
    ac, a_s = _exact_operand(rng, (), m, k, elem_a)
    bc, b_s = _exact_operand(rng, (), n, k, elem_b)
    for blk in (0, 2, 4):
        s1 = a_s.copy()
        s1[3, blk] = 0xFF
        got = _run(dev, ac, s1, bc, b_s, elem_a, elem_b)
        assert np.isnan(got[3]).all() and np.isfinite(np.delete(got, 3, axis=0)).all(), blk
        _same_values(got, _ref(ac, s1, bc, b_s, elem_a, elem_b)[0], ("A scale", blk))
        s2 = b_s.copy()
        s2[11, blk] = 0xFF
        got = _run(dev, ac, a_s, bc, s2, elem_a, elem_b)
        assert np.isnan(got[:, 11]).all() and np.isfinite(np.delete(got, 11, axis=1)).all(), blk
        _same_values(got, _ref(ac, a_s, bc, s2, elem_a, elem_b)[0], ("B scale", blk))
    if elem_a in F.ELEMS:
        ones = np.full_like(ac, 0xFF)                                       # every code 0x3F: the largest magnitude, negative
        sc = np.full_like(a_s, 120)
        got = _run(dev, ones, sc, bc, b_s, elem_a, elem_b)
        assert np.isfinite(got).all()
        _same_values(got, _ref(ones, sc, bc, b_s, elem_a, elem_b)[0], "all-ones codes")


# ------------------------------------------------------------------------------------------------ 5. through the encoder
@pytest.mark.parametrize("elem", F.ELEMS)
@pytest.mark.parametrize("xs,ws", [((34, 96), (96, 24)), ((2, 17, 64), (64, 48))])
def test_random_data_through_the_encoder(dev, elem, xs, ws):
    """test_mx_gemm_gpu.py's data and shapes; |got - ref| <= factor * Kp * 2^-23 * S + 2^-149 against the fp64 product of the decoded
    bytes, the factor this format was measured to need (mx_verify.BOUND_FACTOR: 1 where the measured ratio is 0, else twice the worst
    one)."""
    from dipoorlet_amd import ops
    from dipoorlet_amd.mx_verify import BOUND_FACTOR
    rng = np.random.default_rng(xs[0] * 100 + ws[1])
    x, w = rng.standard_normal(xs).astype(np.float32), rng.standard_normal(ws).astype(np.float32)
    x[..., 5] *= 40.0
    x[..., ws[0] - 3] *= 90.0
    w[7] *= 25.0
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    w_codes, w_scales = ops.mx_encode(wd, 0, elem)
    kp = 32 * -(-ws[0] // 32)
    assert tuple(w_codes.shape) == (ws[1], kp * 3 // 4)
    got = ops.mx_matmul(xd, w_codes, w_scales, elem).cpu().numpy()
    assert got.shape == xs[:-1] + (ws[1],)
    x_codes, x_scales = ops.mx_encode(xd, -1, elem)
    assert np.array_equal(x_codes.cpu().numpy(), F.encode(x, -1, elem)[0]) and np.array_equal(w_codes.cpu().numpy(), F.encode(w, 0, elem)[0])
    ref, s = _ref(x_codes.cpu().numpy(), x_scales.cpu().numpy(), w_codes.cpu().numpy(), w_scales.cpu().numpy(), elem, elem)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ratio = float((err / (kp * 2.0 ** -23 * s + 2.0 ** -149)).max())
    print(f"mx_gemm through the encoder {elem} {xs} x {ws}: max |got - ref| / (Kp 2^-23 S) = {ratio:.4g}")
    assert not np.isnan(got).any() and (err <= G.bound(s, kp, BOUND_FACTOR[elem])).all(), ratio
    want = torch.matmul(ops.fake_quant_mx(xd, -1, elem).double(), ops.fake_quant_mx(wd, 0, elem).double()).cpu().numpy()
    assert (np.abs(got - want) <= G.bound(s, kp, BOUND_FACTOR[elem])).all()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(dev):
    import ctypes as C

    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    rng = np.random.default_rng(5)
    ac, a_s = _exact_operand(rng, (), 8, 64, "mxfp6_e2m3")
    bc, b_s = _exact_operand(rng, (), 6, 64, "mxfp6_e3m2")
    a, sa, b, sb = (torch.from_numpy(x).to(dev) for x in (ac, a_s, bc, b_s))
    out = torch.full((8, 6), -777.0, dtype=torch.float32, device=dev)
    for args, pat in (((a, sa, b, sb, "mxfp6"), r"'mxfp8' or 'mxfp4'"), ((a, sa, b, sb, "mxfp6_e2m3", "mxfp6_e2m5"), r"'mxfp6_e2m3' / 'mxfp6_e3m2'"),
                      ((a, sa, b, sb, "mxfp8", "mxfp6_e3m2"), r"A must be codes \[.*Kp\]"),          # 48 bytes a row are not 64 E4M3 codes
                      ((a, sa, b, sb, "mxfp6_e2m3", "mxfp4"), r"B must be codes"),
                      ((a, sa, b[:, :24].contiguous(), sb, "mxfp6_e2m3"), r"B must be codes \[.*Kp \* 3 / 4\]")):
        with pytest.raises(_hip.DipoorletHipError, match=pat):
            ops.mx_gemm(*args, out=out) if len(args) == 6 else ops.mx_gemm(*args, None, out)
    ref = torch.zeros(8, 6, device=dev)
    with pytest.raises(_hip.DipoorletHipError, match=r"'mxfp8' or 'mxfp4' \(--mx_mixed"):
        ops.mx_gemm_err(a, sa, b, sb, ref, "mxfp6_e2m3", "mxfp6_e3m2")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    part = torch.zeros(2, dtype=torch.float64, device=dev)
    big = torch.zeros(8 * 48 + 32, dtype=torch.uint8, device=dev)
    pa, psa, pb, psb, pc, pref, ppart = (C.c_void_p(t.data_ptr()) for t in (a, sa, b, sb, out, ref, part))
    for bad in (2, 5, 8):
        assert lib.dpl_mx_gemm(bad, 6, pa, psa, pb, psb, 1, 8, 6, 64, 0, pc, st) == -2 and b"DPL_MX_E2M3 / DPL_MX_E3M2" in lib.dpl_last_error()
        assert lib.dpl_mx_gemm(7, bad, pa, psa, pb, psb, 1, 8, 6, 64, 0, pc, st) == -2 and b"elem_a and elem_b" in lib.dpl_last_error()
    for ea, eb in ((6, 0), (1, 7), (6, 7)):
        assert lib.dpl_mx_gemm_err(ea, eb, pa, psa, pb, psb, 1, 8, 6, 64, 0, pref, None, ppart, st) == -2
        assert b"elem_a and elem_b must be DPL_MX_E4M3 or DPL_MX_E2M1" in lib.dpl_last_error()
    for shift in (4, 8):                                                    # (8: where a block lies, not where the base may)
        mis = C.c_void_p(big.data_ptr() + shift)
        assert lib.dpl_mx_gemm(6, 7, mis, psa, pb, psb, 1, 8, 6, 64, 0, pc, st) == -2 and b"16-byte aligned" in lib.dpl_last_error()
    torch.cuda.synchronize()
    assert (out == -777.0).all() and (part == 0).all(), "a refused call launched"
