"""No GPU: the numpy definition of the OCP Microscaling Q/DQ (tests/mx_model.py) against brute force and against itself, and the
host side of `--mx`: which tensors quant_graph block-scales and under which names, the node to_model writes, the CLI's refusals,
the binding.  The kernel is held to the model in tests/test_mx_gpu.py."""
import types

import numpy as np
import pytest

import mx_model as M

ELEMS = ("mxfp8", "mxfp4")


# ------------------------------------------------------------------------------------------------ 1. the element rounding
def _nearest_code_bruteforce(v):
    """Nearest of the 8 E2M1 codes in fp64; of two equally near, the one with the even code index (= the even mantissa)."""
    c = M.E2M1_CODES.astype(np.float64)
    a = np.minimum(np.abs(np.asarray(v, np.float64)), 8.0)      # (above 7 the nearest code is 6 whatever the value: keeps a - c exact)
    d = np.abs(a[:, None] - c[None, :])                         # exact: fp32 values up to 8 against codes with 2 significant bits
    best = d.min(axis=1, keepdims=True)
    near = d == best
    idx = np.where(near.sum(1) == 1, near.argmax(1), [next((i for i in np.flatnonzero(r) if i % 2 == 0), 0) for r in near])
    return np.copysign(c[idx], v)


def _finite(bits):
    x = bits.astype(np.uint32).view(np.float32)
    return x[np.isfinite(x)]


def test_e2m1_round_against_brute_force():
    rng = np.random.default_rng(3)
    pts = M.boundary_points("mxfp4")
    assert pts.size > 80 and {0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0} <= set(np.abs(pts).tolist())
    rnd = _finite(rng.integers(0, 2 ** 32, 100000, dtype=np.uint64))
    near = rng.integers(0x3E000000, 0x41800000, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)      # 0.125 .. 16
    for x in (pts, rnd, near, -near):
        got, want = M.e2m1_round(x), _nearest_code_bruteforce(x)
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(x))
    table = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0, 6.5: 6.0, 1e9: 6.0, np.inf: 6.0}
    for v, w in table.items():
        assert M.e2m1_round(np.float32(v)) == w and M.e2m1_round(np.float32(-v)) == -w
    z = M.e2m1_round(np.array([0.0, -0.0, -0.2, np.nan], np.float32))
    assert np.signbit(z).tolist()[:3] == [False, True, True] and z[2] == 0 and np.isnan(z[3])


# ------------------------------------------------------------------------------------------------ 2. the shared exponent
def _exponent_from_bits(a):
    b = int(np.float32(a).view(np.uint32)) & 0x7FFFFFFF
    field = b >> 23
    return field - 127 if field else b.bit_length() - 1 - 149


def test_shared_exponent_three_ways():
    rng = np.random.default_rng(4)
    a = np.abs(_finite(rng.integers(0, 2 ** 32, 20000, dtype=np.uint64)))
    a = np.concatenate([a[a > 0], np.float32(2.0) ** np.arange(-149, 128, dtype=np.float64).astype(np.float32).astype(np.float64)]).astype(np.float32)
    a = a[a > 0]
    by_bits = np.array([_exponent_from_bits(v) for v in a])
    assert np.array_equal(M.floor_log2(a), by_bits)                                   # np.frexp against the bit field
    for elem in ELEMS:
        assert np.array_equal(M.shared_exponent(a, elem), np.maximum(by_bits - M.EMAX[elem], -127))
    one, below = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0))
    assert M.shared_exponent(one, "mxfp4") == -2 and M.shared_exponent(one, "mxfp8") == -8
    assert M.shared_exponent(below, "mxfp4") == -3 and M.shared_exponent(below, "mxfp8") == -9
    sub = np.float32(2.0 ** -130)                                                     # an fp32 subnormal: its true exponent
    assert M.floor_log2(sub) == -130 and M.floor_log2(np.float32(1.5 * 2.0 ** -140)) == -140 and M.floor_log2(np.float32(1e-45)) == -149
    for elem in ELEMS:                                                                # the clamp at -127
        assert M.shared_exponent(sub, elem) == -127 and M.shared_exponent(np.float32(0), elem) == -127
        e = M.EMAX[elem]
        assert M.shared_exponent(np.float32(2.0 ** (-127 + e)), elem) == -127 and M.shared_exponent(np.float32(2.0 ** (-126 + e)), elem) == -126
        assert M.shared_exponent(np.float32(3.4e38), elem) == 127 - e


# ------------------------------------------------------------------------------------------------ 3. blocks
@pytest.mark.parametrize("elem", ELEMS)
def test_partial_last_block_is_a_block_of_its_own(elem):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 33)) * np.exp(rng.standard_normal((3, 33)) * 3)).astype(np.float32)
    x[:, 32] *= 1000                                       # the 33rd element would change the first block's scale if it were in it
    y, s = M.fake_quant_mx(x, 1, elem, return_scales=True)
    y0, s0 = M.fake_quant_mx(x[:, :32], 1, elem, return_scales=True)
    y1, s1 = M.fake_quant_mx(x[:, 32:], 1, elem, return_scales=True)
    assert s.shape == (3, 2, 1) and np.array_equal(y, np.concatenate([y0, y1], 1)) and np.array_equal(s, np.concatenate([s0, s1], 1))
    # along a strided axis: the same numbers, transposed
    yt, st = M.fake_quant_mx(x.T.copy(), 0, elem, return_scales=True)
    assert st.shape == (1, 2, 3) and np.array_equal(yt, y.T) and np.array_equal(st[0], s[:, :, 0].T)
    assert np.array_equal(M.fake_quant_mx(x.T.copy(), -2, elem), yt)


@pytest.mark.parametrize("elem", ELEMS)
def test_special_values(elem):
    top, emax = M.ELEM_MAX[elem], M.EMAX[elem]
    ordinary = np.linspace(-3, 3, 32).astype(np.float32)
    want_ordinary = M.fake_quant_mx(ordinary[None], 1, elem)[0]
    x = np.tile(ordinary, (8, 2)).astype(np.float32)       # [8, 64]: block 0 special, block 1 ordinary
    x[0, :32] = 0
    x[0, 1:32:2] = -0.0
    x[1, 7] = np.nan
    x[2, 9] = np.inf
    x[3, 11] = -np.inf
    x[4, :32] = np.float32(2.0 ** -131)
    x[4, 0] = np.float32(2.0 ** -130)                      # a subnormal maximum: se = -127
    x[5, :32] = np.float32(2.0 ** -127)
    x[5, 0] = np.float32(2.0 ** -120)
    x[6, :32] = np.float32(1.0)
    x[6, 0] = np.float32(3.4028234663852886e38)            # the largest finite fp32
    y, s = M.fake_quant_mx(x, 1, elem, return_scales=True)
    assert np.array_equal(y[:, 32:], np.tile(want_ordinary, (8, 1)))          # the ordinary block beside each: untouched
    assert (y[0, :32] == 0).all() and np.array_equal(np.signbit(y[0, :32]), np.signbit(x[0, :32])) and s[0, 0, 0] == 0
    for r in (1, 2, 3):
        assert np.isnan(y[r, :32]).all() and s[r, 0, 0] == 0xFF and s[r, 1, 0] != 0xFF
    # a = 2^-130: se = -127; under X = 2^-127 the values are 2^-3 and 2^-4 — codes of E4M3, below half a step of E2M1
    assert s[4, 0, 0] == 0 and y[4, :2].tolist() == ([2.0 ** -130, 2.0 ** -131] if elem == "mxfp8" else [0.0, 0.0])
    # a = 2^-120: E4M3 clamps (-128 -> -127) and 2^-127 comes out as 1 * 2^-127, a subnormal OUTPUT; E2M1: se = -122, 2^-5 -> 0
    assert s[5, 0, 0] == max(-120 - emax, -127) + 127 and y[5, 0] == np.float32(2.0 ** -120)
    assert y[5, 1] == (np.float32(2.0 ** -127) if elem == "mxfp8" else 0)
    assert s[6, 0, 0] == 127 - emax + 127 and y[6, 0] == np.float32(top * 2.0 ** (127 - emax)) and np.isfinite(y[6]).all()
    # a an exact power of two and its two fp32 neighbours: the lower neighbour falls into the binade below
    for a, se in ((np.float32(1.0), -emax), (np.nextafter(np.float32(1.0), np.float32(2)), -emax), (np.nextafter(np.float32(1.0), np.float32(0)), -emax - 1)):
        blk = np.full((1, 32), 0.3, np.float32)
        blk[0, 0] = a
        y1, s1 = M.fake_quant_mx(blk, 1, elem, return_scales=True)
        assert s1[0, 0, 0] == se + 127
        assert y1[0, 0] == (1.0 if a >= 1 else top * 2.0 ** (-emax - 1))     # below 1: saturates at the largest value of the lower binade


@pytest.mark.parametrize("elem", ELEMS)
def test_invariant_under_power_of_two_scaling(elem):
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((16, 96)) * np.exp(rng.standard_normal((16, 96)) * 2)).astype(np.float32)
    y, s = M.fake_quant_mx(x, 1, elem, return_scales=True)
    assert s.min() > 90 and s.max() < 140
    for p in (-90, -13, 1, 60, 100):                      # se + p stays inside [-127, 127], x * 2^p inside fp32's normal range
        f = np.float32(2.0 ** p)
        yp, sp = M.fake_quant_mx(x * f, 1, elem, return_scales=True)
        assert np.array_equal(yp, y * f) and np.array_equal(sp.astype(np.int64), s.astype(np.int64) + p)


# ------------------------------------------------------------------------------------------------ 4. quant_graph
def _hand_graph():
    """A Conv; its output read by a MatMul AND, after it, by a second Conv (one tensor with an MX and a static consumer); a MatMul
    of an activation with a constant; a second MatMul that reads the first one's activation `t` along its other axis; a Gemm with
    transB and a bias."""
    from dipoorlet_amd.models import _B
    g = _B(9)
    x = g.conv("input", 3, 4, 3, 1, 1, "c1")                                   # [1, 4, 6, 6]
    g.node("MatMul", [x, g.w("w2", (6, 3), fan_in=6)], out="m0")               # c1_out along -1, w2 along -2
    g.conv(x, 4, 2, 1, 1, 0, "c2")                                             # ... and the static consumer of c1_out
    t = g.node("Reshape", [x, g.const("shape_t", np.array([1, 4, 36], np.int64))], out="t")
    w1 = g.w("w1", (36, 8), fan_in=36)
    m1 = g.node("MatMul", [t, w1], out="m1")                                   # t along -1, w1 along -2
    m2 = g.node("MatMul", [g.node("Transpose", [m1], out="m1_t", perm=[0, 2, 1]), t], out="m2")   # m1_t along -1, t along -2
    f = g.node("Flatten", [m2], out="flat", axis=1)                            # [1, 288]
    wg = g.w("wg", (5, 288))
    out = g.node("Gemm", [f, wg, g.b("bg", 5)], out="output", alpha=1.0, beta=1.0, transB=1)
    return g.finish("input", [1, 3, 6, 6], out)


def _clip(g):
    names = ["input", "c1_out", "c2_out", "m0", "t", "m1", "m1_t", "m2", "flat", "output"]
    clip = {n: [np.float32(-1.0), np.float32(2.0)] for n in names}
    for w in ("c1.weight", "c2.weight", "wg"):
        a = g.get_initializer(w).reshape(g.get_initializer(w).shape[0], -1)
        clip[w] = [a.min(1), a.max(1)]
    return clip


def _fq_nodes(gq):
    return [(n.name, n.input[0], n.output[0], gq._qdq[n.name].fmt, gq._qdq[n.name].block_axis) for n in gq.graph.node if n.op_type == "FakeQuant"]


def test_quant_graph_block_scales_matmul_and_gemm_operands():
    from dipoorlet_amd.quantize import quant_graph
    g = _hand_graph()
    base, _ = quant_graph(g, _clip(g), types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[]))
    none, _ = quant_graph(g, _clip(g), types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx=None))
    assert _fq_nodes(base) == _fq_nodes(none) and [(n.op_type, n.input, n.output) for n in base.graph.node] == \
        [(n.op_type, n.input, n.output) for n in none.graph.node]
    # today: activations of MatMul / Gemm and the Gemm weight are static E4M3, a MatMul constant is left in fp32
    static = ("input", "c1.weight", "c1_out", "c2.weight", "t", "m1_t", "flat", "wg")
    assert [(i, f) for _, i, _, f, _ in _fq_nodes(base)] == [(t, "Float8E4M3FN") for t in static]
    assert set(base.initializer) - set(g.initializer) == {f"{t}_{k}" for t in static for k in ("scale", "zero_point")}
    assert not any("_static" in n.name for n in base.graph.node)
    for fmt, typ in (("mxfp4", "MXFP4E2M1"), ("mxfp8", "MXFP8E4M3")):
        gq, qlist = quant_graph(g, _clip(g), types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx=fmt))
        assert [n.op_type for n in qlist] == ["Conv", "MatMul", "Conv", "MatMul", "MatMul", "Gemm"]
        assert _fq_nodes(gq) == [
            ("input_QuantizeLinear", "input", "input_dq", "Float8E4M3FN", None),              # the Conv keeps E4M3, both operands
            ("c1.weight_QuantizeLinear", "c1.weight", "c1.weight_dq", "Float8E4M3FN", None),
            ("c1_out_QuantizeLinear", "c1_out", "c1_out_dq", typ, -1),                        # the MatMul comes first: the usual names
            ("w2_QuantizeLinear", "w2", "w2_dq", typ, -2),
            ("c1_out_QuantizeLinear_static", "c1_out", "c1_out_dq_static", "Float8E4M3FN", None),   # ... the second Conv's static pair
            ("c2.weight_QuantizeLinear", "c2.weight", "c2.weight_dq", "Float8E4M3FN", None),
            ("t_QuantizeLinear", "t", "t_dq", typ, -1),                                       # MatMul A
            ("w1_QuantizeLinear", "w1", "w1_dq", typ, -2),                                    # MatMul's constant B: no role before
            ("m1_t_QuantizeLinear", "m1_t", "m1_t_dq", typ, -1),
            ("t_QuantizeLinear_ax-2", "t", "t_dq_ax-2", typ, -2),                             # the same tensor along its other axis
            ("flat_QuantizeLinear", "flat", "flat_dq", typ, 1),                               # Gemm A
            ("wg_QuantizeLinear", "wg", "wg_dq", typ, 1),                                     # Gemm B, transB
        ]
        by_out = {n.output[0]: n for n in gq.graph.node}
        assert by_out["m0"].input == ["c1_out_dq", "w2_dq"] and by_out["c2_out"].input == ["c1_out_dq_static", "c2.weight_dq", "c2.bias"]
        assert by_out["m1"].input == ["t_dq", "w1_dq"] and by_out["m2"].input == ["m1_t_dq", "t_dq_ax-2"]
        assert by_out["output"].input == ["flat_dq", "wg_dq", "bg"]                           # the bias is left alone
        # an MX node brings no scale / zero-point initializers
        assert set(gq.initializer) - set(g.initializer) == {"input_scale", "input_zero_point", "c1.weight_scale", "c1.weight_zero_point",
                                                            "c1_out_scale_static", "c1_out_zero_point_static", "c2.weight_scale",
                                                            "c2.weight_zero_point"}
    # Gemm without transB, with transA: the other axes
    from dipoorlet_amd.onnx_io import Node
    from dipoorlet_amd.quantize import mx_block_axis
    assert [mx_block_axis(Node("Gemm", ["a", "b"], ["c"], attrs=at), i, None) for at in ({}, {"transA": 1, "transB": 1}) for i in (0, 1)] == [1, 0, 0, 1]
    assert mx_block_axis(Node("MatMul", ["a", "b"], ["c"]), 1, [7]) == -1 and mx_block_axis(Node("MatMul", ["a", "b"], ["c"]), 1, [7, 3]) == -2


def test_to_model_writes_the_custom_node_and_it_round_trips(tmp_path):
    from dipoorlet_amd import onnx_io
    from dipoorlet_amd.quantize import quant_graph
    g = _hand_graph()
    gq, _ = quant_graph(g, _clip(g), types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx="mxfp4"))
    m = gq.to_model()
    mx = [n for n in m.nodes if n.op_type == "MXQuantizeDequantize"]
    assert [(n.name, n.input, n.output, n.domain, n.attrs) for n in mx] == [
        (f"{t}_QuantizeLinear{sfx}", [t], [f"{t}_dq{sfx}"], "dipoorlet.amd", {"axis": ax, "block_size": 32, "elem_type": "float4e2m1"})
        for t, sfx, ax in (("c1_out", "", -1), ("w2", "", -2), ("t", "", -1), ("w1", "", -2), ("m1_t", "", -1), ("t", "_ax-2", -2), ("flat", "", 1), ("wg", "", 1))]
    assert m.opset["dipoorlet.amd"] == 1 and m.opset[""] >= 19                      # (19: the Conv's float8e4m3fn pairs)
    assert not any(n.op_type == "FakeQuant" for n in m.nodes)
    assert sum(n.op_type == "QuantizeLinear" for n in m.nodes) == 4 == sum(n.op_type == "DequantizeLinear" for n in m.nodes)
    pair = [n for n in m.nodes if n.name in ("c1_out_QuantizeLinear_static", "c1_out_DequantizeLinear_static")]
    assert [(n.op_type, n.input, n.output) for n in pair] == [
        ("QuantizeLinear", ["c1_out", "c1_out_scale_static", "c1_out_zero_point_static"], ["c1_out_q_static"]),
        ("DequantizeLinear", ["c1_out_q_static", "c1_out_scale_static", "c1_out_zero_point_static"], ["c1_out_dq_static"])]
    path = str(tmp_path / "mx.onnx")
    onnx_io.save_model(m, path)
    back = onnx_io.load_model(path)
    assert back.opset["dipoorlet.amd"] == 1 and back.opset[""] == m.opset[""]
    got = [(n.name, list(n.input), list(n.output), n.domain, dict(n.attrs)) for n in back.nodes if n.op_type == "MXQuantizeDequantize"]
    assert got == [(n.name, n.input, n.output, n.domain, n.attrs) for n in mx]
    m8 = quant_graph(g, _clip(g), types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx="mxfp8"))[0].to_model()
    assert {n.attrs["elem_type"] for n in m8.nodes if n.op_type == "MXQuantizeDequantize"} == {"float8e4m3fn"}
    # without --mx: no trace of the domain
    plain = quant_graph(g, _clip(g), types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[]))[0].to_model()
    assert "dipoorlet.amd" not in plain.opset and not any(n.domain for n in plain.nodes)


def test_emitter_lists_the_mx_tensors(tmp_path):
    import json

    from dipoorlet_amd.deploy import to_deploy
    g = _hand_graph()
    clip = _clip(g)
    act = {k: [float(v[0]), float(v[1])] for k, v in clip.items() if k not in ("c1.weight", "c2.weight", "wg")}
    wt = {k: clip[k] for k in ("c1.weight", "c2.weight", "wg")}
    to_deploy(g, act, wt, types.SimpleNamespace(deploy="ocp_fp8", output_dir=str(tmp_path), skip_layers=[], mx="mxfp8"))
    blocks = json.load(open(tmp_path / "ocp_mx_blocks.json"))
    assert blocks == {"format": "mxfp8", "block_size": 32, "tensors": {
        "c1_out": {"axis": -1, "constant": False}, "w2": {"axis": -2, "constant": True},
        "t": {"axis": -1, "constant": False}, "w1": {"axis": -2, "constant": True}, "m1_t": {"axis": -1, "constant": False},
        "t_ax-2": {"axis": -2, "constant": False}, "flat": {"axis": 1, "constant": False}, "wg": {"axis": 1, "constant": True}}}
    assert set(json.load(open(tmp_path / "ocp_fp8_scales.json"))["scale"]) == set(act)
    plain = tmp_path / "plain"
    plain.mkdir()
    to_deploy(g, act, wt, types.SimpleNamespace(deploy="ocp_fp8", output_dir=str(plain), skip_layers=[], mx=None))
    assert [p.name for p in plain.iterdir()] == ["ocp_fp8_scales.json"]
    assert open(plain / "ocp_fp8_scales.json").read() == open(tmp_path / "ocp_fp8_scales.json").read()


# ------------------------------------------------------------------------------------------------ 5. CLI, table, binding
def _parse(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", *extra])


@pytest.mark.parametrize("deploy", ["trt", "stpu", "magicmind", "rv", "atlas", "snpe", "ti", "imx"])
def test_cli_refuses_mx_on_every_other_platform(deploy):
    from dipoorlet_amd.__main__ import check_args
    with pytest.raises(ValueError) as e:
        check_args(_parse("-D", deploy, "-A", "hist", "--mx", "mxfp4"))
    assert "--mx mxfp4" in str(e.value) and f"-D {deploy}" in str(e.value) and "-D ocp_fp8" in str(e.value)
    check_args(_parse("-D", deploy, "-A", "hist"))          # and without --mx nothing has changed


def test_cli_accepts_mx_with_ocp_fp8_and_keeps_its_refusals():
    from dipoorlet_amd.__main__ import check_args
    assert _parse("-D", "ocp_fp8").mx is None
    for fmt in ELEMS:
        check_args(_parse("-D", "ocp_fp8", "-A", "hist", "--mx", fmt, "--smooth", "--bc", "--we", "--update_bn"))
    for flags in (["-A", "mse"], ["-A", "kl"], ["-A", "hist", "--adaround"], ["-A", "hist", "--brecq"], ["-A", "minmax", "--sparse"]):
        with pytest.raises(ValueError, match="floating-point grid"):
            check_args(_parse("-D", "ocp_fp8", "--mx", "mxfp8", *flags))
    with pytest.raises(SystemExit):
        _parse("-D", "ocp_fp8", "--mx", "mxfp6")


def test_mx_is_no_platform():
    from dipoorlet_amd.platform_settings import mx_setting_table, platform_setting_table
    assert len(platform_setting_table) == 9
    assert mx_setting_table == {"mxfp8": {"bit_width": 8, "type": "MXFP8E4M3", "block_size": 32},
                                "mxfp4": {"bit_width": 4, "type": "MXFP4E2M1", "block_size": 32}}
    from dipoorlet_amd.quantize import get_qnode_by_param
    for fmt, top in (("mxfp8", 448), ("mxfp4", 6)):
        q, lo, hi = get_qnode_by_param(mx_setting_table[fmt], "t", [2, 64], None, block_axis=-1)       # `range` is ignored
        assert q.is_mx and q.block_axis == -1 and (lo, hi) == (-top, top) == q.saturation() and q.output == "t_dq"


def test_binding_declares_the_entry_point():
    import ctypes as C

    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 27
    p, u64 = C.c_void_p, C.c_uint64
    assert _hip.SIGNATURES["dpl_fake_quant_mx"] == (C.c_int, [C.c_int32, p, p, u64, u64, u64, p, p])
    assert (_hip.MX_E4M3, _hip.MX_E2M1) == (0, 1)
