"""GPU: the block-scaled convolution of `--mx_conv` (k_mx_conv; dpl_mx_conv, ops.mx_conv) against the numpy definition
(tests/mx_conv_model.py).  The lane map is k_mx_gemm's (tests/test_mx_gemm_gpu.py holds it); what is new is the tap addressing, and
test 1 does not take it on trust: every image holds ONE non-zero element and every weight element differs, so every output is 0 or
one product — a swapped ky and kx, a tap paired with the wrong pixel, a channel block with the wrong scale byte or a wrong stride,
pad or dilation each change some output — and asks for bit equality.  Test 2 draws data whose every partial sum is exact in fp32 in
any order (elements 0, +-1, +-2, +-3, +-4, +-6, scale bytes 125 .. 129: every product a multiple of 2^-4, asserted on the CPU to sum
below 2^24 such units) at the shapes where the kernel masks rows, columns, taps and K-blocks.  Test 3: a 1 x 1 convolution IS
ops.mx_gemm, bit for bit.  Only test 4 (random data through the encoder) has a tolerance: mx_gemm_model.bound with Kp = kh * kw * 32
* Cb, factor 1 for mxfp4 and mx_gemm_model.HW_FACTOR for mxfp8."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import mx_conv_model as CM
import mx_gemm_model as G

pytestmark = pytest.mark.gpu

ELEMS = ("mxfp8", "mxfp4")
PAIRS = [(a, b) for a in ELEMS for b in ELEMS]
GUARD = 64           # floats around C
SENTINEL = -777.0
EXACT_VALUES = np.array([0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6], np.float64)
NONZERO = np.array([0.5, 1, 1.5, 2, 3, 4, 6])                   # values of E2M1 and of E4M3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _geometry(h, w, kh, kw, strides, pads, dil):
    """pads = (top, left), applied at the end of each axis too -> the keyword arguments of ops.mx_conv / mx_conv_model.mx_conv."""
    oh = CM.out_size(h, kh, strides[0], pads[0], pads[0], dil[0])
    ow = CM.out_size(w, kw, strides[1], pads[1], pads[1], dil[1])
    return dict(strides=tuple(strides), pads=tuple(pads), dilations=tuple(dil), out_hw=(oh, ow))


def _exact_operand(rng, lead, c, elem):
    """Codes and scales of [*lead, Cp] exact-class data; the channels past c are pad: code 0."""
    cp = 32 * -(-c // 32)
    v = rng.choice(EXACT_VALUES, size=tuple(lead) + (cp,))
    v[..., c:] = 0.0
    return G.codes_from_values(v, elem), rng.integers(125, 130, size=tuple(lead) + (cp // 32,)).astype(np.uint8)


def _run(dev, ac, a_s, bc, b_s, elem_a, elem_b, geo):
    """ops.mx_conv into a C with a guard band on both sides -> the result on the host (the band is checked)."""
    from dipoorlet_amd import ops
    shape = (ac.shape[0],) + tuple(geo["out_hw"]) + (bc.shape[0],)
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    out = buf[GUARD:GUARD + numel].view(shape)
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (ac, a_s, bc, b_s)]
    assert ops.mx_conv(*t, elem_a, elem_b, out=out, **geo) is out
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + numel:] == SENTINEL).all(), "the guard band around C was written"
    return host[GUARD:GUARD + numel].reshape(shape)


def _same_values(got, want, what):
    """Equal as values (a zero's sign is free), NaN in the same places."""
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~wn & (got != want)))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), [float(got[tuple(i)]) for i in bad[:5]], [float(want[tuple(i)]) for i in bad[:5]])


# ------------------------------------------------------------------------------------------------ 1. the tap map, exact
# image b holds ONE element, at (y, x, channel): a corner, the right edge, the interior, the bottom edge; channel block 0 and the
# short block 1 (channels 32 .. 39); both parities
SPOTS = [(0, 0, 5), (2, 4, 38), (3, 2, 33), (5, 1, 12)]
TAP_GEOMETRIES = [((1, 1), (1, 1), (1, 1)), ((2, 1), (1, 0), (1, 1)), ((1, 1), (0, 2), (1, 2))]      # (strides, pads, dilations)


def _tap_map_case():
    n, c, h, w, cout, k = 4, 40, 6, 5, 16, 3
    a = np.zeros((n, h, w, 64))
    for b, (y, x, ch) in enumerate(SPOTS):
        a[b, y, x, ch] = NONZERO[(3 * b + 2) % 7] * (-1 if b % 2 else 1)
    co, ky, kx, ch = np.meshgrid(np.arange(cout), np.arange(k), np.arange(k), np.arange(64), indexing="ij")
    bv = NONZERO[(5 * co + 3 * ky + kx + 2 * ch + (ch >> 5)) % 7] * np.where((co + 2 * ky + kx + ch // 3) % 2 == 1, -1.0, 1.0)
    bv[..., c:] = 0.0
    nn, yy, xx, blk = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(2), indexing="ij")
    a_s = (118 + (7 * nn + 3 * yy + 5 * xx + 11 * blk) % 17).astype(np.uint8)                      # differ per (pixel, block)
    co, ky, kx, blk = np.meshgrid(np.arange(cout), np.arange(k), np.arange(k), np.arange(2), indexing="ij")
    b_s = (119 + (5 * co + 7 * ky + 3 * kx + 13 * blk) % 19).astype(np.uint8)                      # ... per (co, tap, block)
    return a, a_s, bv, b_s


@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_tap_map_is_exact(dev, elem_a, elem_b):
    a, a_s, bv, b_s = _tap_map_case()
    assert {ch // 32 for *_, ch in SPOTS} == {0, 1} and {ch % 2 for *_, ch in SPOTS} == {0, 1}
    assert all((np.diff(s.astype(np.int64), axis=ax) != 0).all() for s in (a_s, b_s) for ax in range(4))      # neighbours differ along every axis
    ac, bc = G.codes_from_values(a, elem_a), G.codes_from_values(bv, elem_b)
    for strides, pads, dil in TAP_GEOMETRIES:
        geo = _geometry(6, 5, 3, 3, strides, pads, dil)
        want, _ = CM.mx_conv(ac, a_s, bc, b_s, elem_a, elem_b, **geo)
        # every output is 0 or ONE product a 2^(sa - 127) * b 2^(sb - 127), exact in fp32: written out per image
        one = np.zeros(want.shape)
        for b, (y, x, ch) in enumerate(SPOTS):
            for ky in range(3):
                for kx in range(3):
                    ny, nx = y + pads[0] - ky * dil[0], x + pads[1] - kx * dil[1]
                    if ny % strides[0] == 0 and nx % strides[1] == 0 and 0 <= ny // strides[0] < geo["out_hw"][0] and 0 <= nx // strides[1] < geo["out_hw"][1]:
                        e = int(a_s[b, y, x, ch // 32]) + b_s[:, ky, kx, ch // 32].astype(np.int64) - 254
                        one[b, ny // strides[0], nx // strides[1], :] = a[b, y, x, ch] * bv[:, ky, kx, ch] * 2.0 ** e
        assert np.array_equal(want.astype(np.float64), one) and all((want[b] != 0).any() for b in range(4)), (strides, pads, dil)
        # ... and not symmetric: under ky <-> kx of the weight, nor under oy <-> ox (on the largest square both axes have)
        swapped = CM.mx_conv(ac, a_s, bc.transpose(0, 2, 1, 3), b_s.transpose(0, 2, 1, 3), elem_a, elem_b, **geo)[0]
        assert not np.array_equal(swapped, want)
        sq = min(geo["out_hw"])
        assert not np.array_equal(want[:, :sq, :sq], want[:, :sq, :sq].transpose(0, 2, 1, 3))
        got = _run(dev, ac, a_s, bc, b_s, elem_a, elem_b, geo)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, ((strides, pads, dil), len(bad), bad[:8].tolist(), got[tuple(bad[:8].T)].tolist(), want[tuple(bad[:8].T)].tolist())


# ------------------------------------------------------------------------------------------------ 2. the exact class
# (n, c, h, w, cout, k, stride, pad, dilation)
SHAPES = [(2, 40, 7, 6, 20, 3, 2, 1, 1),
          (1, 3, 9, 9, 8, 7, 2, 3, 1),          # C = 3: one short block
          (3, 128, 4, 4, 70, 1, 1, 0, 1),       # Cb = 4, cout crosses a tile, m < 64
          (1, 32, 11, 11, 16, 3, 1, 2, 2),      # 121 rows cross a tile, dilation
          (2, 64, 9, 9, 33, 3, 1, 1, 1)]        # 18 K-blocks: a last step of two


@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_exact_class_at_every_masking_shape(dev, elem_a, elem_b):
    rng = np.random.default_rng(len(elem_a) * 11 + len(elem_b))
    for n, c, h, w, cout, k, stride, pad, dil in (SHAPES if elem_a == elem_b else SHAPES[:2]):
        ac, a_s = _exact_operand(rng, (n, h, w), c, elem_a)
        bc, b_s = _exact_operand(rng, (cout, k, k), c, elem_b)
        geo = _geometry(h, w, k, k, (stride, stride), (pad, pad), (dil, dil))
        want, s = CM.mx_conv(ac, a_s, bc, b_s, elem_a, elem_b, **geo)
        # every product is a multiple of 2^(125 + 125 - 254) = 2^-4: sums below 2^24 such units are exact in fp32 in any order
        assert float(s.max()) < 2.0 ** 24 * 2.0 ** -4 and (want != 0).any()
        got = _run(dev, ac, a_s, bc, b_s, elem_a, elem_b, geo)
        _same_values(got, want, (n, c, h, w, cout, k, stride, pad, dil))


# ------------------------------------------------------------------------------------------------ 3. 1 x 1 is the GEMM
@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_one_by_one_is_mx_gemm(dev, elem_a, elem_b):
    from dipoorlet_amd import ops
    rng = np.random.default_rng(31)
    x = torch.from_numpy(rng.standard_normal((2, 70, 9, 8)).astype(np.float32)).to(dev)
    wt = torch.from_numpy(rng.standard_normal((72, 70, 1, 1)).astype(np.float32)).to(dev)
    ac, a_s = ops.mx_encode(x, 1, elem_a)
    bc, b_s = ops.mx_encode(wt, 1, elem_b)
    assert tuple(a_s.shape) == (2, 9, 8, 3) and tuple(b_s.shape) == (72, 1, 1, 3)
    got = ops.mx_conv(ac, a_s, bc, b_s, elem_a, elem_b, strides=(1, 1), pads=(0, 0), dilations=(1, 1), out_hw=(9, 8))
    want = ops.mx_gemm(ac.reshape(2, 72, -1), a_s.reshape(2, 72, -1), bc.reshape(72, -1), b_s.reshape(72, -1), elem_a, elem_b)
    assert tuple(got.shape) == (2, 9, 8, 72) and torch.isfinite(got).all() and (got != 0).any()
    assert torch.equal(got.reshape(2, 72, 72).view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 4. through the encoder
# |got - ref| <= factor * Kp * 2^-23 * S + 2^-149 (mx_gemm_model.bound), Kp = kh * kw * 32 * Cb: factor 1 for mxfp4 (exact products,
# fp32 additions in any order) and mx_gemm_model.HW_FACTOR for mxfp8 (the instruction truncates the E4M3 products of every run of 8
# consecutive k before it adds them: DESIGN.md §3o).  The worst ratios measured are in DESIGN.md §3r.
BOUND_FACTOR = {"mxfp4": 1.0, "mxfp8": G.HW_FACTOR}


@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(41)
    x, wt = rng.standard_normal((2, 40, 9, 9)).astype(np.float32), rng.standard_normal((24, 40, 3, 3)).astype(np.float32)
    x[:, 5] *= 40.0                                                       # a few large channels
    x[:, 37] *= 90.0
    wt[7] *= 25.0
    return x, wt


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("stride", [1, 2])
def test_random_data_through_the_encoder(dev, random_case, elem, stride):
    from dipoorlet_amd import ops
    x, wt = random_case
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(wt).to(dev)
    ac, a_s = ops.mx_encode(xd, 1, elem)
    bc, b_s = ops.mx_encode(wd, 1, elem)
    geo = _geometry(9, 9, 3, 3, (stride, stride), (1, 1), (1, 1))
    got = ops.mx_conv(ac, a_s, bc, b_s, elem, **geo).cpu().numpy()
    ref, s = CM.mx_conv(ac.cpu().numpy(), a_s.cpu().numpy(), bc.cpu().numpy(), b_s.cpu().numpy(), elem, **geo)
    kp = 3 * 3 * 64
    assert got.shape == ref.shape == (2,) + geo["out_hw"] + (24,)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ratio = float((err / (kp * 2.0 ** -23 * s + 2.0 ** -149)).max())
    print(f"mx_conv through the encoder {elem} stride {stride}: max |got - ref| / (Kp 2^-23 S) = {ratio:.4g}")
    assert not np.isnan(got).any() and (err <= G.bound(s, kp, BOUND_FACTOR[elem])).all(), ratio
    # and it is torch's fp32 convolution of the decoded operands, to twice that bound (that side carries an fp32 summation too)
    a_hat = ops.mx_decode(ac, a_s, elem, (2, 64, 9, 9), 1)
    b_hat = ops.mx_decode(bc, b_s, elem, (24, 64, 3, 3), 1)
    want = torch.nn.functional.conv2d(a_hat, b_hat, None, stride, 1).permute(0, 2, 3, 1).cpu().numpy()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"  against torch's fp32 convolution: {float((err / (2 * G.bound(s, kp, BOUND_FACTOR[elem]))).max()):.4g} of twice the bound")
    assert (err <= 2 * G.bound(s, kp, BOUND_FACTOR[elem])).all()


# ------------------------------------------------------------------------------------------------ 5. the NaN rule
@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_nan_rule(dev, elem_a, elem_b):
    rng = np.random.default_rng(23)
    ac, a_s = _exact_operand(rng, (2, 6, 6), 40, elem_a)
    bc, b_s = _exact_operand(rng, (5, 3, 3), 40, elem_b)
    geo = _geometry(6, 6, 3, 3, (1, 1), (1, 1), (1, 1))
    # a 0xFF scale byte at pixel (3, 2) of image 1: exactly the outputs whose in-image taps reach it
    for blk in (0, 1):
        s1 = a_s.copy()
        s1[1, 3, 2, blk] = 0xFF
        got = _run(dev, ac, s1, bc, b_s, elem_a, elem_b, geo)
        reach = np.zeros(got.shape, bool)
        reach[1, 2:5, 1:4, :] = True
        assert np.array_equal(np.isnan(got), reach), blk
        _same_values(got, CM.mx_conv(ac, s1, bc, b_s, elem_a, elem_b, **geo)[0], ("A scale", blk))
    s1 = a_s.copy()
    s1[0, 0, 5, 1] = 0xFF                                                  # a corner: four outputs
    got = _run(dev, ac, s1, bc, b_s, elem_a, elem_b, geo)
    assert np.isnan(got[0, :2, 4:, :]).all() and np.isnan(got).sum() == 4 * 5
    # the same pixel under a 1 x 1 stride-2 convolution that skips it: everything finite
    b1c, b1s = _exact_operand(rng, (5, 1, 1), 40, elem_b)
    g2 = _geometry(6, 6, 1, 1, (2, 2), (0, 0), (1, 1))
    s1 = a_s.copy()
    s1[1, 3, 2, 0] = 0xFF
    got = _run(dev, ac, s1, b1c, b1s, elem_a, elem_b, g2)
    assert np.isfinite(got).all()
    _same_values(got, CM.mx_conv(ac, s1, b1c, b1s, elem_a, elem_b, **g2)[0], "skipped by stride 2")
    # the weight: a 0xFF byte or an E4M3 NaN code anywhere in row co makes channel co NaN everywhere and nothing else
    s2 = b_s.copy()
    s2[3, 2, 0, 1] = 0xFF
    got = _run(dev, ac, a_s, bc, s2, elem_a, elem_b, geo)
    assert np.isnan(got[..., 3]).all() and np.isfinite(np.delete(got, 3, axis=-1)).all()
    if elem_b == "mxfp8":
        for code, at in ((0x7F, (1, 0, 0, 2)), (0xFF, (1, 2, 2, 39))):
            c1 = bc.copy()
            c1[at] = code
            z = ac.copy()
            z[..., at[3] // 2 if elem_a == "mxfp4" else at[3]] = 0       # against zeros of A at that channel: still NaN
            got = _run(dev, z, a_s, c1, b_s, elem_a, elem_b, geo)
            assert np.isnan(got[..., 1]).all() and np.isfinite(np.delete(got, 1, axis=-1)).all(), (code, at)
    if elem_a == "mxfp8":
        c1 = ac.copy()
        c1[0, 4, 4, 35] = 0x7F
        got = _run(dev, c1, a_s, bc, b_s, elem_a, elem_b, geo)
        reach = np.zeros(got.shape, bool)
        reach[0, 3:6, 3:6, :] = True
        assert np.array_equal(np.isnan(got), reach)
        _same_values(got, CM.mx_conv(c1, a_s, bc, b_s, elem_a, elem_b, **geo)[0], "A code")


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(dev):
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    rng = np.random.default_rng(5)
    ac, a_s = _exact_operand(rng, (1, 4, 4), 64, "mxfp8")
    bc, b_s = _exact_operand(rng, (6, 3, 3), 64, "mxfp8")
    a, sa, b, sb = (torch.from_numpy(x).to(dev) for x in (ac, a_s, bc, b_s))
    out = torch.full((1, 4, 4, 6), SENTINEL, dtype=torch.float32, device=dev)
    geo = dict(strides=(1, 1), pads=(1, 1), dilations=(1, 1), out_hw=(4, 4))
    for args, kw, pat in (((a, sa, b, sb, "mxfp6"), {}, r"'mxfp8' or 'mxfp4'"), ((a, sa, b, sb, "mxfp8", "e5m2"), {}, r"'mxfp8' or 'mxfp4'"),
                          ((a, sa, b[..., :32].contiguous(), sb, "mxfp8"), {}, r"B must be codes"),             # 32 codes against 2 scale bytes
                          ((a, sa, b[..., :32].contiguous(), sb[..., :1].contiguous(), "mxfp8"), {}, r"same number of K-blocks"),
                          ((a, sa, b, sb, "mxfp4"), {}, r"must be codes"),                                      # fp8 bytes are not Cp / 2 nibble pairs
                          ((a, sa[:, :3].contiguous(), b, sb, "mxfp8"), {}, r"A must be codes"),
                          ((a[0], sa[0], b, sb, "mxfp8"), {}, r"A must be codes"),                              # no batch dimension
                          ((a.cpu(), sa, b, sb, "mxfp8"), {}, r"no CPU path"), ((a, sa.int(), b, sb, "mxfp8"), {}, r"uint8"),
                          ((a, sa, b, sb, "mxfp8"), {"strides": (1,)}, r"strides must be two integers"),
                          ((a, sa, b, sb, "mxfp8"), {"pads": (1.0, 1)}, r"pads must be two integers"),
                          ((a, sa, b, sb, "mxfp8"), {"out_hw": (4, -4)}, r"out_hw must not be negative"),
                          ((a, sa, b, sb, "mxfp8"), {"strides": (0, 1)}, r"at least 1"), ((a, sa, b, sb, "mxfp8"), {"dilations": (1, 0)}, r"at least 1"),
                          ((a, sa, b, sb, "mxfp8"), {"pads": (-1, 1)}, r"must not be negative"),
                          ((a, sa, b, sb, "mxfp8"), {"strides": (1 << 31, 1)}, r"2\^31")):
        with pytest.raises(_hip.DipoorletHipError, match=pat):
            ops.mx_conv(*args, out=out, **{**geo, **kw})
    with pytest.raises(_hip.DipoorletHipError, match=r"out must have shape \[1, 4, 4, 6\]"):
        ops.mx_conv(a, sa, b, sb, "mxfp8", out=torch.empty(1, 6, 4, 4, device=dev), **geo)
    # the C ABI: (n, h, w, c, cout, kh, kw, sh, sw, pt, pl, dh, dw, oh, ow)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    big = torch.zeros(ac.size + 32, dtype=torch.uint8, device=dev)
    pa, psa, pb, psb, pc, pbig = (C.c_void_p(t.data_ptr()) for t in (a, sa, b, sb, out, big))
    ok = [1, 4, 4, 64, 6, 3, 3, 1, 1, 1, 1, 1, 1, 4, 4]
    names = ["n", "h", "w", "c", "cout", "kh", "kw", "sh", "sw", "pt", "pl", "dh", "dw", "oh", "ow"]

    def call(pa_=pa, psa_=psa, pb_=pb, psb_=psb, pc_=pc, ea=0, eb=0, **change):
        dims = list(ok)
        for k, v in change.items():
            dims[names.index(k)] = v
        return lib.dpl_mx_conv(ea, eb, pa_, psa_, pb_, psb_, *dims, pc_, st)
    assert call(ea=2) == -2 and b"elem" in lib.dpl_last_error()
    assert call(eb=-1) == -2 and b"elem" in lib.dpl_last_error()
    for p in ("pa_", "psa_", "pb_", "psb_", "pc_"):
        assert call(**{p: None}) == -2 and b"null" in lib.dpl_last_error(), p
    for k in ("kh", "kw", "sh", "sw", "dh", "dw"):
        for v in (0, -1):
            assert call(**{k: v}) == -2 and b"at least 1" in lib.dpl_last_error(), (k, v)
    for k in ("pt", "pl"):
        assert call(**{k: -1}) == -2 and b"negative" in lib.dpl_last_error(), k
    for k in names:
        assert call(**{k: 1 << 31}) == -2 and b"2^31" in lib.dpl_last_error(), k
    for k in ("n", "h", "w", "c", "cout", "oh", "ow"):
        assert call(**{k: -1}) == -2 and b"2^31" in lib.dpl_last_error(), k
    top = (1 << 31) - 1
    assert call(kh=top, kw=top) == -2 and b"too large" in lib.dpl_last_error()                     # the K-blocks of a weight row
    assert call(oh=top, ow=top) == -2 and b"too large" in lib.dpl_last_error()                     # the output pixels of an image
    assert call(n=top, h=top, w=top, c=top) == -2 and b"too large" in lib.dpl_last_error()         # A's bytes
    assert call(cout=top, kh=1 << 20, kw=1 << 10, c=top) == -2 and b"too large" in lib.dpl_last_error()
    assert call(n=top, oh=1 << 15, ow=1 << 15, cout=top) == -2 and b"too large" in lib.dpl_last_error()        # C's bytes
    assert call(n=1 << 20, oh=1 << 10, ow=1 << 10) == -2 and b"the grid" in lib.dpl_last_error()
    for k in ("n", "h", "w", "c", "cout", "oh", "ow"):
        assert call(None, None, None, None, None, 1, 1, **{k: 0}) == 0, k
    for shift in (1, 4, 8):
        mis = C.c_void_p(big.data_ptr() + shift)
        assert call(pa_=mis) == -2 and b"16-byte aligned" in lib.dpl_last_error()
        assert call(pb_=mis) == -2 and b"16-byte aligned" in lib.dpl_last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call launched"
    assert call(pa_=pbig) == 0                                                                     # and on a boundary it runs
    torch.cuda.synchronize()
    assert (out == 0).all()
