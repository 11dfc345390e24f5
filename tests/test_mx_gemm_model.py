"""No GPU: the definition of the block-scaled product (tests/mx_gemm_model.py) against cases worked by hand, its NaN rule, the pad
codes, and what `--mx_verify` declares: the flag's refusal, the ABI version and the entry point's signature."""
import os
import re

import numpy as np
import pytest

import mx_gemm_model as G
import mx_pack_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMS = ("mxfp8", "mxfp4")
PAIRS = [(a, b) for a in ELEMS for b in ELEMS]


def _hand_case():
    """2 x 2 x 32 in values both element formats hold.  A (scales 2, 1/2): row 0 = 1 at k 0, -2 at k 1; row 1 = 3 at k 5, 0.5 at
    k 31.  B (scales 1, 4): row 0 = 4 at k 0, 1 at k 1, 6 at k 31; row 1 = -1 at k 0, 2 at k 5."""
    a, b = np.zeros((2, 32)), np.zeros((2, 32))
    a[0, 0], a[0, 1], a[1, 5], a[1, 31] = 1, -2, 3, 0.5
    b[0, 0], b[0, 1], b[0, 31], b[1, 0], b[1, 5] = 4, 1, 6, -1, 2
    a_s, b_s = np.array([[128], [126]], np.uint8), np.array([[127], [129]], np.uint8)
    # C[0,0] = 2*4 + (-4)*1 = 4; C[0,1] = 2*(-4) = -8; C[1,0] = 0.25*6 = 1.5; C[1,1] = 1.5*8 = 12
    c = np.array([[4.0, -8.0], [1.5, 12.0]], np.float32)
    s = np.array([[12.0, 8.0], [1.5, 12.0]])
    return a, a_s, b, b_s, c, s


@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_model_against_a_case_worked_by_hand(elem_a, elem_b):
    a, a_s, b, b_s, want, want_s = _hand_case()
    ac, bc = G.codes_from_values(a, elem_a), G.codes_from_values(b, elem_b)
    assert ac.shape == (2, 32 if elem_a == "mxfp8" else 16) and bc.shape == (2, 32 if elem_b == "mxfp8" else 16)
    if elem_a == "mxfp8":
        assert (ac[0, 0], ac[0, 1], ac[1, 5], ac[1, 31]) == (0x38, 0xC0, 0x44, 0x30)        # 1, -2, 3, 0.5 as E4M3FN bytes
    else:
        assert (ac[0, 0], ac[1, 2], ac[1, 15]) == (0x2 | (0xC << 4), 0x5 << 4, 0x1 << 4)     # even index low, odd index high
    c, s = G.mx_gemm(ac, a_s, bc, b_s, elem_a, elem_b)
    assert c.dtype == np.float32 and np.array_equal(c, want) and np.array_equal(s, want_s)
    # a batch of A against one B, and against a B per batch
    c3, _ = G.mx_gemm(np.stack([ac, ac, ac]), np.stack([a_s, a_s, a_s]), bc, b_s, elem_a, elem_b)
    assert np.array_equal(c3, np.stack([want] * 3))
    swap = np.stack([bc, bc[::-1]]), np.stack([b_s, b_s[::-1]])
    c2, _ = G.mx_gemm(np.stack([ac, ac]), np.stack([a_s, a_s]), *swap, elem_a, elem_b)
    assert np.array_equal(c2, np.stack([want, want[:, ::-1]]))


def test_model_is_the_decoded_product():
    rng = np.random.default_rng(3)
    x, w = rng.standard_normal((5, 70)).astype(np.float32), rng.standard_normal((70, 9)).astype(np.float32)
    for elem in ELEMS:
        xc, xs = P.encode(x, 1, elem)
        wc, ws = P.encode(w, 0, elem)
        assert wc.shape[0] == 9 and xs.shape == (5, 3) and ws.shape == (9, 3)
        c, s = G.mx_gemm(xc, xs, wc, ws, elem)
        xh, wh = P.decode(xc, xs, elem, x.shape, 1).astype(np.float64), P.decode(wc, ws, elem, w.shape, 0).astype(np.float64)
        assert np.array_equal(c, (xh @ wh).astype(np.float32)) and np.allclose(s, np.abs(xh) @ np.abs(wh), rtol=1e-15)
        assert (G.bound(s, 96) > 0).all()


@pytest.mark.parametrize("elem_a,elem_b", PAIRS)
def test_nan_rule(elem_a, elem_b):
    a, a_s, b, b_s, want, _ = _hand_case()
    a, b = np.tile(a, (2, 1)), np.tile(b, (2, 1))                       # 4 x 4 x 32
    a_s, b_s = np.tile(a_s, (2, 1)), np.tile(b_s, (2, 1))
    ac, bc = G.codes_from_values(a, elem_a), G.codes_from_values(b, elem_b)
    s1 = a_s.copy()
    s1[3, 0] = 0xFF                                                     # a scale byte of A: the row of C
    c, s = G.mx_gemm(ac, s1, bc, b_s, elem_a, elem_b)
    assert np.isnan(c[3]).all() and np.isnan(s[3]).all() and not np.isnan(c[:3]).any()
    s2 = b_s.copy()
    s2[1, 0] = 0xFF                                                     # of B: the column
    c, _ = G.mx_gemm(ac, a_s, bc, s2, elem_a, elem_b)
    assert np.isnan(c[:, 1]).all() and not np.isnan(np.delete(c, 1, axis=1)).any()
    if elem_a == "mxfp8":
        for code in (0x7F, 0xFF):
            c1 = ac.copy()
            c1[2, 17] = code                                            # against a ZERO of B: still NaN
            c, _ = G.mx_gemm(c1, a_s, bc, b_s, elem_a, elem_b)
            assert np.isnan(c[2]).all() and not np.isnan(np.delete(c, 2, axis=0)).any()
    if elem_b == "mxfp8":
        c1 = bc.copy()
        c1[0, 9] = 0x7F
        c, _ = G.mx_gemm(ac, a_s, c1, b_s, elem_a, elem_b)
        assert np.isnan(c[:, 0]).all() and not np.isnan(c[:, 1:]).any()
    if elem_a == "mxfp4":                                               # E2M1 has no NaN code: every nibble is a number
        c1 = ac.copy()
        c1[2, 8] = 0xFF
        assert not np.isnan(G.mx_gemm(c1, a_s, bc, b_s, elem_a, elem_b)[0]).any()


@pytest.mark.parametrize("elem", ELEMS)
def test_pad_codes_are_summed(elem):
    x, w = np.ones((1, 33), np.float32), np.ones((33, 1), np.float32)
    xc, xs = P.encode(x, 1, elem)
    wc, ws = P.encode(w, 0, elem)
    assert xs.shape == (1, 2) and not xc[0, (33 if elem == "mxfp8" else 17):].any()       # the encoder's pad: code 0
    assert G.mx_gemm(xc, xs, wc, ws, elem)[0][0, 0] == 33.0
    pad = G.codes_from_values(np.r_[1.0, 2.0, np.zeros(30)], elem)                          # second block: 1 (k 32), 2 (k 33: pad)
    xc[0, -pad.size:], wc[0, -pad.size:] = pad, pad
    xs[0, 1] = ws[0, 1] = 127
    assert G.mx_gemm(xc, xs, wc, ws, elem)[0][0, 0] == 32.0 + 1.0 + 4.0


def _cli(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", *extra])


def test_mx_verify_needs_mx_pack():
    from dipoorlet_amd.__main__ import check_args
    with pytest.raises(ValueError, match=r"--mx_verify needs --mx_pack"):
        check_args(_cli("-D", "ocp_fp8", "-A", "hist", "--mx", "mxfp8", "--mx_verify"))
    with pytest.raises(ValueError, match=r"--mx_verify needs --mx_pack"):
        check_args(_cli("-D", "ocp_fp8", "-A", "hist", "--mx_verify"))
    for mx in ELEMS:
        check_args(_cli("-D", "ocp_fp8", "-A", "hist", "--mx", mx, "--mx_pack", "--mx_verify"))
        check_args(_cli("-D", "ocp_fp8", "-A", "hist", "--mx", mx, "--mx_pack", "--mx_verify", "--mx_rotate", "--smooth", "--bc"))
    assert _cli("-D", "ocp_fp8").mx_verify is False


def test_abi_declares_the_kernel():
    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 31
    header = open(os.path.join(ROOT, "include", "dipoorlet_hip.h")).read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION
    assert "dpl_mx_gemm" in _hip.SIGNATURES and re.search(r"\bint dpl_mx_gemm\(", header)
    res, argtypes = _hip.SIGNATURES["dpl_mx_gemm"]
    assert len(argtypes) == 13                     # two elems, four operand arrays, batch, m, n, k, b_batched, d_c, the stream
    build = open(os.path.join(ROOT, "dipoorlet_amd", "csrc", "build.py")).read()
    assert "mx_gemm_kernels.hip" in build and os.path.exists(os.path.join(ROOT, "dipoorlet_amd", "csrc", "mx_gemm_kernels.hip"))
