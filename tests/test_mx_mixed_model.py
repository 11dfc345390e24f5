"""No GPU: the definition of `--mx_mixed` (tests/mx_mixed_model.py) — the per-tile error sums in the kernel's order, and the choice
under the bit budget — and the host side of the flag: the CLI's refusals, the ABI, and quant_graph under a format map."""
import os
import re
import types

import numpy as np
import pytest

import mx_mixed_model as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the partials
@pytest.mark.parametrize("shape", [(1, 1), (8, 6), (64, 64), (3, 130, 65), (2, 2, 70, 9)], ids=str)
@pytest.mark.parametrize("with_bias", [False, True])
def test_partials_are_the_plain_sums(shape, with_bias):
    rng = np.random.default_rng(len(shape) * 100 + shape[-1])
    c, ref = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    bias = rng.standard_normal(shape[-1]).astype(np.float32) if with_bias else None
    p = X.gemm_err_partials(c, ref, bias)
    m, n = shape[-2:]
    assert p.shape == shape[:-2] + (-(-m // 64), -(-n // 64), 2) and p.dtype == np.float64
    d = ((c + bias if with_bias else c) - ref).astype(np.float64)
    # tile by tile against a plain fp64 sum
    for tm in range(p.shape[-3]):
        for tn in range(p.shape[-2]):
            rows, cols = slice(64 * tm, 64 * tm + 64), slice(64 * tn, 64 * tn + 64)
            want_d = (d[..., rows, cols] ** 2).sum((-1, -2))
            want_r = (ref[..., rows, cols].astype(np.float64) ** 2).sum((-1, -2))
            assert np.allclose(p[..., tm, tn, 0], want_d, rtol=1e-12, atol=0) and np.allclose(p[..., tm, tn, 1], want_r, rtol=1e-12, atol=0)
    assert np.isclose(X.relative_error(p), (d ** 2).sum() / (ref.astype(np.float64) ** 2).sum(), rtol=1e-12, atol=0)


def test_the_bias_is_added_in_fp32_before_the_reference_is_subtracted():
    c, bias, ref = np.float32([[1.0]]), np.float32([2.0 ** -24]), np.float32([[1.0]])
    assert X.gemm_err_partials(c, ref, bias)[0, 0, 0] == 0.0                # 1 + 2^-24 rounds to 1 in fp32: d = 0
    c, bias, ref = np.float32([[2.0 ** -24]]), np.float32([1.0]), np.float32([[1.0]])
    assert X.gemm_err_partials(c, ref, bias)[0, 0, 0] == 0.0                # (c + bias) - ref, not c + (bias - ref)
    assert X.gemm_err_partials(np.float32([[3.0]]), np.float32([[1.0]]), np.float32([0.5]))[0, 0].tolist() == [6.25, 1.0]


def test_a_nan_of_c_reaches_its_tile_only():
    c, ref = np.ones((70, 70), np.float32), np.full((70, 70), 2.0, np.float32)
    c[65, 3] = np.nan
    p = X.gemm_err_partials(c, ref)
    assert np.isnan(p[1, 0, 0]) and p[1, 0, 1] == 4.0 * 6 * 64 and np.isfinite(np.delete(p.reshape(4, 2), 2, axis=0)).all()


def _order_case():
    """A tile on which the order of the fp64 additions shows.  d^2 = 2^60 at (row 0, column 0), the FIRST term of lane 0 of wave 0,
    and d^2 = 100 at (0, 16), (1, 0) and (1, 16): that lane's next three terms (i = 0; reg 0, j 1; reg 1, j 0; reg 1, j 1).  The
    spacing of fp64 at 2^60 is 2^8: added to 2^60 one by one, each 100 is rounded away; added to each other first they are 300, and
    2^60 + 300 rounds to 2^60 + 2^8."""
    c, ref = np.zeros((64, 64), np.float32), np.zeros((64, 64), np.float32)
    c[0, 0] = 2.0 ** 30
    c[0, 16] = c[1, 0] = c[1, 16] = 10.0
    return c, ref


def test_the_summation_order_is_visible():
    c, ref = _order_case()
    got = X.gemm_err_partials(c, ref)[0, 0, 0]
    assert got == 2.0 ** 60                                               # the defined order: the three 100s are each lost
    dd, _ = X.gemm_err_terms(c, ref)
    assert float(np.sort(dd.reshape(-1)).sum()) == 2.0 ** 60 + 2.0 ** 8 != got       # smallest first keeps them
    # the same terms at transposed places belong to other lanes and other turns — (0, 1) and (1, 1) are lane 1's, (16, 0) is lane
    # 0's term i = 1 —: lane 1 brings 200 to the first fold, and 2^60 + 200 rounds up
    assert X.gemm_err_partials(c.T.copy(), ref)[0, 0, 0] == 2.0 ** 60 + 2.0 ** 8
    # a lane that met its large term last would keep them too
    late = 0.0
    for v in (100.0, 100.0, 100.0, 2.0 ** 60):
        late += v
    assert late == 2.0 ** 60 + 2.0 ** 8


# ------------------------------------------------------------------------------------------------ choose
def _formats(entries, bits):
    got = X.choose(entries, bits)
    assert list(got) == [e[0] for e in entries] and set(got.values()) <= {"mxfp4", "mxfp8"}
    return [k for k, v in got.items() if v == "mxfp8"]


ENTRIES = [("a", 0.10, 0.01, 100), ("b", 0.30, 0.01, 1000), ("c", 0.05, 0.04, 50), ("d", 0.02, 0.03, 10), ("e", float("nan"), 0.01, 10),
           ("f", 0.2, float("nan"), 10), ("g", 0.5, 0.5, 10), ("h", float("inf"), 0.1, 10)]


def test_choose_at_the_ends_of_the_budget():
    assert _formats(ENTRIES, 4) == []
    assert _formats(ENTRIES, 4.0) == []
    assert _formats(ENTRIES, 8) == ["a", "b", "c"]                        # every node with a positive finite gain, and no other
    assert X.average_bits(ENTRIES, X.choose(ENTRIES, 8)) == pytest.approx(4 + 4 * 1150 / 1200, rel=1e-15) and X.average_bits(ENTRIES, X.choose(ENTRIES, 4)) == 4.0


def test_choose_skips_what_does_not_fit_and_goes_on():
    # gain / cost: a 0.09 / 400, b 0.29 / 4000, c 0.01 / 200 -> a, b, c.  Budget of (5 - 4) * 1200 = 1200 bits: a (400) fits, b
    # (4000) does not and is skipped, c (200) behind it is taken
    assert _formats(ENTRIES, 5) == ["a", "c"]
    assert X.average_bits(ENTRIES, X.choose(ENTRIES, 5)) <= 5
    # exactly enough for a and b: the comparison is <=
    exact = 4 + 4400 / 1200
    assert _formats(ENTRIES, exact + 1e-9) == ["a", "b"] and _formats(ENTRIES, exact - 1e-6) == ["a", "c"]


def test_choose_breaks_ties_in_graph_order():
    tie = [("x", 0.2, 0.1, 100), ("y", 0.2, 0.1, 100), ("z", 0.2, 0.1, 100)]
    assert _formats(tie, 4 + 4 / 3 + 1e-9) == ["x"] and _formats(tie, 4 + 8 / 3 + 1e-9) == ["x", "y"]
    assert _formats(tie[::-1], 4 + 4 / 3 + 1e-9) == ["z"]
    # equal ratio at different sizes is a tie too
    assert _formats([("big", 0.4, 0.0, 200), ("small", 0.2, 0.0, 100)], 4 + 4 * 200 / 300 + 1e-9) == ["big"]
    assert _formats([("small", 0.2, 0.0, 100), ("big", 0.4, 0.0, 200)], 4 + 4 * 200 / 300 + 1e-9) == ["small"]


def test_choose_never_promotes_a_gain_that_is_not_positive():
    for e4, e8 in ((0.1, 0.1), (0.1, 0.2), (float("nan"), 0.1), (0.1, float("nan")), (float("inf"), 0.1), (float("inf"), float("inf")), (0.0, 0.0)):
        assert _formats([("n", e4, e8, 10), ("ok", 0.2, 0.1, 10)], 8) == ["ok"], (e4, e8)


def test_the_package_chooses_as_the_model_does():
    from dipoorlet_amd import mx_mixed
    rng = np.random.default_rng(4)
    for _ in range(50):
        n = int(rng.integers(1, 9))
        entries = [(f"n{i}", float(rng.choice([0.0, 0.1, 0.2, 0.3, np.nan])), float(rng.choice([0.0, 0.05, 0.1, np.nan])), int(rng.choice([32, 64, 4096])))
                   for i in range(n)]
        bits = float(rng.choice([4.0, 4.5, 5.5, 6.0, 8.0]))
        assert mx_mixed.choose(entries, bits) == X.choose(entries, bits), (entries, bits)


# ------------------------------------------------------------------------------------------------ the CLI's rules
def _parse(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", "-D", "ocp_fp8", "-A", "hist", *extra])


def test_cli_rules():
    from dipoorlet_amd.__main__ import check_args
    assert _parse().mx_mixed is None and _parse("--mx", "mxfp4", "--mx_mixed", "5.5").mx_mixed == 5.5
    with pytest.raises(ValueError, match=r"--mx_mixed needs --mx mxfp4"):
        check_args(_parse("--mx_mixed", "5"))
    with pytest.raises(ValueError, match=r"--mx_mixed is not supported with --mx mxfp8"):
        check_args(_parse("--mx", "mxfp8", "--mx_mixed", "5"))
    for bits in ("3.99", "8.01", "-1", "nan", "inf"):
        with pytest.raises(ValueError, match=r"--mx_mixed must lie in \[4, 8\]"):
            check_args(_parse("--mx", "mxfp4", "--mx_mixed", bits))
    for bits in ("4", "5.5", "8"):
        check_args(_parse("--mx", "mxfp4", "--mx_mixed", bits, "--smooth", "--mx_rotate", "--bc", "--we", "--update_bn", "--mx_pack", "--mx_verify",
                          "--mx_scale_search", "--mx_conv"))
    check_args(_parse("--mx", "mxfp4", "--mx_mixed", "6", "--mx_gptq"))


# ------------------------------------------------------------------------------------------------ the binding
def test_binding_and_header_declare_abi_35():
    import ctypes as C

    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 35
    header = open(os.path.join(ROOT, "include", "dipoorlet_hip.h")).read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION
    assert "dpl_mx_gemm_err" in _hip.SIGNATURES and re.search(r"\bint dpl_mx_gemm_err\(", header)
    res, argtypes = _hip.SIGNATURES["dpl_mx_gemm_err"]
    assert res is C.c_int and argtypes == [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_uint64] * 4 + [C.c_int32] + [C.c_void_p] * 4
    decl = re.search(r"\bint dpl_mx_gemm_err\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(argtypes) and decl.count("uint64_t") == 4 and "double* d_part" in decl and "const float* d_ref" in decl
    from dipoorlet_amd.csrc import build as hipbuild
    src = open([p for p in hipbuild.SRC if p.endswith("mx_gemm_kernels.hip")][0]).read()
    assert "k_mx_gemm_err" in src and "atomic" not in src.split("k_mx_gemm_err(", 1)[1].split("extern \"C\"", 1)[0].lower()


# ------------------------------------------------------------------------------------------------ quant_graph under a format map
def _graph():
    """x -> MatMul fc1 -> Relu -> MatMul fc2 -> y; x -> MatMul side (reads x too) -> Add."""
    from dipoorlet_amd.models import _B
    g = _B(3)
    w1, w2, w3 = g.w("fc1.weight", (64, 96)), g.w("fc2.weight", (96, 64)), g.w("side.weight", (64, 64))
    h = g.node("MatMul", ["input", w1], out="h")
    r = g.node("Relu", [h], out="r")
    y = g.node("MatMul", [r, w2], out="y")
    s = g.node("MatMul", ["input", w3], out="s")
    out = g.node("Add", [y, s], out="output")
    return g.finish("input", [1, 5, 64], out)


def _clip(g):
    clip = {n: [np.float32(-1.0), np.float32(2.0)] for n in ("input", "h", "r", "y", "s", "output")}
    for name, w in g.initializer.items():
        clip[name] = [np.asarray(w).min(), np.asarray(w).max()]
    return clip


def _mx_nodes(gq):
    return {n.name: (n.input[0], gq._qdq[n.name].fmt, n.output[0]) for n in gq.graph.node if n.op_type == "FakeQuant" and gq._qdq[n.name].is_mx}


def test_quant_graph_consults_the_format_map():
    from dipoorlet_amd.quantize import quant_graph
    g = _graph()
    name = {n.output[0]: n.name for n in g.graph.node if n.op_type == "MatMul"}       # fc1 -> h, fc2 -> y, side -> s
    fc1, fc2, side = name["h"], name["y"], name["s"]
    args = types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx="mxfp4")
    plain, _ = quant_graph(g, _clip(g), args)
    # a map that promotes nothing is no map: node for node
    same, _ = quant_graph(g, _clip(g), types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx="mxfp4", mx_formats={n: "mxfp4" for n in (fc1, fc2, side)}))
    assert _mx_nodes(plain) == _mx_nodes(same) and {f for _, f, _ in _mx_nodes(plain).values()} == {"MXFP4E2M1"}
    assert [(n.op_type, n.name, list(n.input), list(n.output)) for n in plain.graph.node] == [(n.op_type, n.name, list(n.input), list(n.output)) for n in same.graph.node]
    for promoted in (fc2, fc1, side):
        gq, _ = quant_graph(g, _clip(g), types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx="mxfp4", mx_formats={promoted: "mxfp8"}))
        by_out = {o: (t, f) for t, f, o in _mx_nodes(gq).values()}
        assert len(by_out) == len(_mx_nodes(gq))                          # every MX node has an output of its own
        for node in gq.graph.node:
            if node.op_type == "MatMul":
                want = "MXFP8E4M3" if node.name == promoted else "MXFP4E2M1"
                assert [by_out[i][1] for i in node.input[:2]] == [want, want], (promoted, node.name)
        fmts = sorted(f for _, f in by_out.values())
        # fc2's operands are its own; fc1 and side share `input`, which then has a node of each format
        assert fmts == ["MXFP4E2M1"] * (3 if promoted == fc2 else 4) + ["MXFP8E4M3"] * 2, (promoted, fmts)
        # and the saved model says so
        saved = gq.to_model()
        elem = {n.output[0]: n.attrs["elem_type"] for n in saved.nodes if n.op_type == "MXQuantizeDequantize"}
        assert len(elem) == len(by_out)
        for n in saved.nodes:
            if n.op_type == "MatMul":
                want = "float8e4m3fn" if n.name == promoted else "float4e2m1"
                assert [elem[i] for i in n.input[:2]] == [want, want], (promoted, n.name)
