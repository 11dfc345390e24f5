"""No GPU: the numpy definition of the block-scaled convolution (tests/mx_conv_model.py) against a direct fp64 convolution of the
decoded operands, its NaN rule, its 1 x 1 case against mx_gemm_model; and the host side of `--mx_conv`: the CLI's refusals, which
tensors quant_graph block-scales on a small conv graph and which Convs it leaves, the "conv" entry of ocp_mx_blocks.json, the
binding.  The kernel is held to the model in tests/test_mx_conv_gpu.py."""
import json
import os
import re
import types

import numpy as np
import pytest

import mx_conv_model as CM
import mx_gemm_model as G
import mx_pack_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMS = ("mxfp8", "mxfp4")


def _direct(a, b, strides, pads, dilations, out_hw):
    """a fp64 [n, Cp, h, w], b fp64 [cout, Cp, kh, kw] -> [n, oh, ow, cout]: the convolution written out, one output at a time."""
    n, _, h, w = a.shape
    cout, _, kh, kw = b.shape
    (sh, sw), (pt, pl), (dh, dw), (oh, ow) = strides, pads, dilations, out_hw
    c = np.zeros((n, oh, ow, cout))
    for oy in range(oh):
        for ox in range(ow):
            for ky in range(kh):
                for kx in range(kw):
                    iy, ix = oy * sh - pt + ky * dh, ox * sw - pl + kx * dw
                    if 0 <= iy < h and 0 <= ix < w:
                        c[:, oy, ox, :] += a[:, :, iy, ix] @ b[:, :, ky, kx].T
    return c


# (n, c, h, w, cout, kh, kw, strides, pads (top, left, bottom, right), dilations): stride, asymmetric reach, dilation, C % 32 != 0
GEOMETRIES = [(2, 40, 7, 6, 5, 3, 3, (2, 2), (1, 1, 1, 1), (1, 1)),
              (1, 3, 6, 8, 4, 3, 2, (1, 2), (2, 0, 0, 1), (1, 1)),
              (2, 33, 8, 7, 3, 2, 3, (1, 1), (0, 2, 1, 2), (2, 2)),
              (1, 64, 5, 5, 6, 1, 1, (2, 1), (0, 0, 0, 0), (1, 1))]


@pytest.mark.parametrize("elem_a,elem_b", [(a, b) for a in ELEMS for b in ELEMS])
def test_model_is_the_direct_convolution_of_the_decoded_operands(elem_a, elem_b):
    rng = np.random.default_rng(3)
    for n, c, h, w, cout, kh, kw, strides, pads, dil in GEOMETRIES:
        x = rng.standard_normal((n, c, h, w)).astype(np.float32) * np.exp(rng.standard_normal((1, c, 1, 1))).astype(np.float32)
        wt = rng.standard_normal((cout, c, kh, kw)).astype(np.float32)
        ac, a_s = P.encode(x, 1, elem_a)
        bc, b_s = P.encode(wt, 1, elem_b)
        cb = -(-c // 32)
        assert ac.shape == (n, h, w, cb * (32 if elem_a == "mxfp8" else 16)) and a_s.shape == (n, h, w, cb)
        assert bc.shape == (cout, kh, kw, cb * (32 if elem_b == "mxfp8" else 16)) and b_s.shape == (cout, kh, kw, cb)
        if c % 32:                                        # the pad codes take part: give some a value
            ac[..., -1], bc[..., -1] = 0x22, 0x33
        oh = CM.out_size(h, kh, strides[0], pads[0], pads[2], dil[0])
        ow = CM.out_size(w, kw, strides[1], pads[1], pads[3], dil[1])
        got, s = CM.mx_conv(ac, a_s, bc, b_s, elem_a, elem_b, strides=strides, pads=pads[:2], dilations=dil, out_hw=(oh, ow))
        a = P.decode(ac, a_s, elem_a, (n, 32 * cb, h, w), 1).astype(np.float64)
        b = P.decode(bc, b_s, elem_b, (cout, 32 * cb, kh, kw), 1).astype(np.float64)
        want = _direct(a, b, strides, pads[:2], dil, (oh, ow))
        assert got.shape == (n, oh, ow, cout) and got.dtype == np.float32
        tol = 1e-12 * _direct(np.abs(a), np.abs(b), strides, pads[:2], dil, (oh, ow)) + 1e-300
        assert (np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)) <= 2.0 ** -23 * np.abs(want) + tol).all()
        assert np.allclose(s, _direct(np.abs(a), np.abs(b), strides, pads[:2], dil, (oh, ow)), rtol=1e-12, atol=0)
        if c % 32:
            zero = CM.mx_conv(np.where(np.arange(ac.shape[-1]) == ac.shape[-1] - 1, 0, ac).astype(np.uint8), a_s, bc, b_s, elem_a, elem_b,
                              strides=strides, pads=pads[:2], dilations=dil, out_hw=(oh, ow))[0]
            assert (zero != got).any(), "the pad codes did not take part"


def _exact(rng, lead, c, elem):
    cp = 32 * -(-c // 32)
    v = rng.choice(np.array([0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6], np.float64), size=tuple(lead) + (cp,))
    v[..., c:] = 0.0
    return G.codes_from_values(v, elem), rng.integers(125, 130, size=tuple(lead) + (cp // 32,)).astype(np.uint8)


@pytest.mark.parametrize("elem", ELEMS)
def test_nan_rule_on_constructed_bytes(elem):
    rng = np.random.default_rng(5)
    ac, a_s = _exact(rng, (1, 6, 6), 40, elem)
    bc, b_s = _exact(rng, (4, 3, 3), 40, elem)
    geo = dict(strides=(1, 1), pads=(1, 1), dilations=(1, 1), out_hw=(6, 6))
    clean, _ = CM.mx_conv(ac, a_s, bc, b_s, elem, **geo)
    assert np.isfinite(clean).all()
    s1 = a_s.copy()
    s1[0, 3, 2, 1] = 0xFF                                       # pixel (3, 2), its short block: reached by outputs (2..4, 1..3)
    got, s = CM.mx_conv(ac, s1, bc, b_s, elem, **geo)
    reach = np.zeros((1, 6, 6, 4), bool)
    reach[0, 2:5, 1:4, :] = True
    assert np.array_equal(np.isnan(got), reach) and np.array_equal(np.isnan(s), reach) and np.array_equal(got[~reach], clean[~reach])
    s1 = a_s.copy()
    s1[0, 0, 0, 0] = 0xFF                                       # a corner: reached by (0..1, 0..1) only
    reach[:] = False
    reach[0, :2, :2, :] = True
    assert np.array_equal(np.isnan(CM.mx_conv(ac, s1, bc, b_s, elem, **geo)[0]), reach)
    # a 1 x 1 stride-2 convolution skips the odd pixels: a bad one there leaves everything finite, a bad even one its own output
    b1c, b1s = _exact(rng, (4, 1, 1), 40, elem)
    g2 = dict(strides=(2, 2), pads=(0, 0), dilations=(1, 1), out_hw=(3, 3))
    s1 = a_s.copy()
    s1[0, 3, 2, 0] = 0xFF
    assert np.isfinite(CM.mx_conv(ac, s1, b1c, b1s, elem, **g2)[0]).all()
    s1[0, 4, 2, 0] = 0xFF
    got = CM.mx_conv(ac, s1, b1c, b1s, elem, **g2)[0]
    assert np.isnan(got[0, 2, 1]).all() and np.isnan(got).sum() == 4
    # the weight: any block of row co makes channel co NaN everywhere, nothing else
    s2 = b_s.copy()
    s2[2, 0, 2, 1] = 0xFF
    got = CM.mx_conv(ac, a_s, bc, s2, elem, **geo)[0]
    assert np.isnan(got[..., 2]).all() and np.isfinite(np.delete(got, 2, axis=-1)).all()
    if elem == "mxfp8":
        for code in (0x7F, 0xFF):
            c1 = bc.copy()
            c1[1, 2, 0, 39] = code
            got = CM.mx_conv(ac, a_s, c1, b_s, elem, **geo)[0]
            assert np.isnan(got[..., 1]).all() and np.isfinite(np.delete(got, 1, axis=-1)).all()
            c1 = ac.copy()
            c1[0, 5, 5, 3] = code
            assert np.isnan(CM.mx_conv(c1, a_s, bc, b_s, elem, **geo)[0]).sum() == 4 * 4


@pytest.mark.parametrize("elem_a,elem_b", [(a, b) for a in ELEMS for b in ELEMS])
def test_one_by_one_is_the_gemm_model(elem_a, elem_b):
    rng = np.random.default_rng(8)
    x, wt = rng.standard_normal((3, 70, 4, 5)).astype(np.float32), rng.standard_normal((9, 70, 1, 1)).astype(np.float32)
    ac, a_s = P.encode(x, 1, elem_a)
    bc, b_s = P.encode(wt, 1, elem_b)
    a_s[1, 2, 3, 1] = 0xFF
    got, s = CM.mx_conv(ac, a_s, bc, b_s, elem_a, elem_b, strides=(1, 1), pads=(0, 0), dilations=(1, 1), out_hw=(4, 5))
    want, sw = G.mx_gemm(*CM.as_gemm(ac, a_s, bc, b_s), elem_a, elem_b)
    assert np.array_equal(got.reshape(3, 20, 9), want, equal_nan=True) and np.isnan(got).sum() == 9
    assert np.allclose(s.reshape(3, 20, 9), sw, rtol=1e-14, atol=0, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the CLI's rules
def _parse(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", *extra])


def test_cli_rules():
    from dipoorlet_amd.__main__ import check_args
    assert _parse("-D", "ocp_fp8").mx_conv is False
    with pytest.raises(ValueError, match=r"--mx_conv needs --mx"):
        check_args(_parse("-D", "ocp_fp8", "-A", "hist", "--mx_conv"))
    with pytest.raises(ValueError, match=r"--mx_conv and --mx_gptq"):
        check_args(_parse("-D", "ocp_fp8", "-A", "hist", "--mx", "mxfp4", "--mx_conv", "--mx_gptq"))
    for fmt in ELEMS:
        check_args(_parse("-D", "ocp_fp8", "-A", "hist", "--mx", fmt, "--mx_conv", "--smooth", "--bc", "--we", "--update_bn", "--mx_rotate",
                          "--mx_scale_search", "--mx_pack", "--mx_verify"))


# ------------------------------------------------------------------------------------------------ quant_graph
def _conv_graph():
    """ca reads the input; its output `ca_out` is read by two taken Convs (3 x 3 and 1 x 1) and by a grouped one."""
    from dipoorlet_amd.models import _B
    g = _B(4)
    x = g.conv("input", 8, 40, 3, 1, 1, "ca")
    y1 = g.conv(x, 40, 16, 3, 1, 1, "cb")
    y2 = g.conv(x, 40, 16, 1, 1, 0, "cc")
    y3 = g.conv(x, 40, 16, 3, 1, 1, "cg", groups=4)
    out = g.node("Add", [g.node("Add", [y1, y2], out="s12"), y3], out="output")
    return g.finish("input", [1, 8, 6, 6], out)


def _clip(g):
    clip = {n: [np.float32(-1.0), np.float32(2.0)] for n in ("input", "ca_out", "cb_out", "cc_out", "cg_out", "s12", "output")}
    for name, w in g.initializer.items():
        a = np.asarray(w).reshape(w.shape[0], -1)
        clip[name] = [a.min(1), a.max(1)]
    return clip


def _args(**kw):
    return types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], **kw)


def _fq(gq):
    return [(n.name, list(n.input), list(n.output), gq._qdq[n.name].fmt, gq._qdq[n.name].block_axis) for n in gq.graph.node if n.op_type == "FakeQuant"]


def test_quant_graph_block_scales_the_eligible_convs():
    from dipoorlet_amd.quantize import MX_NODES, mx_block_axis, quant_graph
    assert MX_NODES == ["MatMul", "Gemm"]
    g = _conv_graph()
    # without the flag: today's graph, node for node — every Conv operand on the static grid
    today, _ = quant_graph(g, _clip(g), _args(mx="mxfp4"))
    off, _ = quant_graph(g, _clip(g), _args(mx="mxfp4", mx_conv=False))
    assert _fq(today) == _fq(off) and [(n.op_type, n.name, n.input, n.output) for n in today.graph.node] == \
        [(n.op_type, n.name, n.input, n.output) for n in off.graph.node]
    assert {f for *_, f, _ in _fq(off)} == {"Float8E4M3FN"} and set(today.initializer) == set(off.initializer)
    for fmt, typ in (("mxfp4", "MXFP4E2M1"), ("mxfp8", "MXFP8E4M3")):
        gq, _ = quant_graph(g, _clip(g), _args(mx=fmt, mx_conv=True))
        nodes = {n.name: n for n in gq.graph.node}
        mx = [(i[0], ax) for _, i, _, f, ax in _fq(gq) if f == typ]
        # one MXQuantizeDequantize per (tensor, axis 1): ca_out, read by two taken Convs, has one
        assert sorted(mx) == sorted([("input", 1), ("ca.weight", 1), ("ca_out", 1), ("cb.weight", 1), ("cc.weight", 1)])
        convs = {n.name: n for n in gq.graph.node if n.op_type == "Conv"}
        by_w = {n.input[1].split("_dq")[0]: n for n in convs.values()}
        assert by_w["cb.weight"].input[0] == by_w["cc.weight"].input[0] == "ca_out_dq"
        assert all(mx_block_axis(n, i, None) == 1 for n in convs.values() for i in (0, 1))
        # the grouped Conv keeps static nodes on both operands: a second, static node of ca_out and its own weight's
        static = {i[0]: (name, o[0]) for name, i, o, f, _ in _fq(gq) if f == "Float8E4M3FN"}
        cg = by_w["cg.weight"]
        assert cg.input[0] == static["ca_out"][1] == "ca_out_dq_static" and cg.input[1] == static["cg.weight"][1]
        assert static["ca_out"][0] in nodes
        # and the saved model says the same
        saved = gq.to_model()
        got = sorted((n.input[0], n.attrs["axis"], n.attrs["block_size"]) for n in saved.nodes if n.op_type == "MXQuantizeDequantize")
        assert got == sorted((t, 1, 32) for t, _ in mx)


def test_emitter_lists_the_taken_and_the_left_convs(tmp_path):
    from dipoorlet_amd.deploy import to_deploy
    g = _conv_graph()
    clip = _clip(g)
    act = {k: [float(v[0]), float(v[1])] for k, v in clip.items() if k not in g.initializer}
    wt = {k: v for k, v in clip.items() if k in g.initializer}
    to_deploy(g, act, wt, types.SimpleNamespace(deploy="ocp_fp8", output_dir=str(tmp_path), skip_layers=[], mx="mxfp8", mx_conv=True))
    blocks = json.load(open(tmp_path / "ocp_mx_blocks.json"))
    by_weight = {n.input[1]: n.name for n in g.graph.node if n.op_type == "Conv"}
    assert blocks["conv"] == {"nodes": [by_weight[w] for w in ("ca.weight", "cb.weight", "cc.weight")], "left": {by_weight["cg.weight"]: "group = 4"}}
    assert blocks["tensors"] == {"input": {"axis": 1, "constant": False}, "ca.weight": {"axis": 1, "constant": True},
                                 "ca_out": {"axis": 1, "constant": False}, "cb.weight": {"axis": 1, "constant": True},
                                 "cc.weight": {"axis": 1, "constant": True}}
    plain = tmp_path / "plain"
    plain.mkdir()
    to_deploy(g, act, wt, types.SimpleNamespace(deploy="ocp_fp8", output_dir=str(plain), skip_layers=[], mx="mxfp8"))
    assert "conv" not in json.load(open(plain / "ocp_mx_blocks.json")) and json.load(open(plain / "ocp_mx_blocks.json"))["tensors"] == {}


def test_reasons_a_conv_is_left():
    from dipoorlet_amd.models import _B
    from dipoorlet_amd.onnx_io import Node
    from dipoorlet_amd.quantize import mx_conv_left
    g = _B(1)
    x = g.conv("input", 4, 4, 3, 1, 1, "c2d")
    g.w("w1d", (4, 4, 3))
    g.nodes.append(Node("Conv", [x, "w1d"], ["o1"], name="conv1d", attrs={"group": 1}))
    g.nodes.append(Node("Conv", [x, x], ["o2"], name="dyn", attrs={"group": 1}))
    graph = g.finish("input", [1, 4, 5, 5], "o2")
    by = {n.name: n for n in graph.graph.node}
    assert mx_conv_left(graph, by["conv1d"]) == "a 1-D convolution" and mx_conv_left(graph, by["dyn"]) == "the weight is not a constant"
    assert [mx_conv_left(graph, n) for n in graph.graph.node if n.op_type == "Conv" and n.input[1] == "c2d.weight"] == [None]


# ------------------------------------------------------------------------------------------------ the binding
def test_binding_and_header_declare_abi_34():
    import ctypes as C

    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 34
    header = open(os.path.join(ROOT, "include", "dipoorlet_hip.h")).read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION
    assert "dpl_mx_conv" in _hip.SIGNATURES and re.search(r"\bint dpl_mx_conv\(", header)
    res, argtypes = _hip.SIGNATURES["dpl_mx_conv"]
    assert res is C.c_int and argtypes == [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int64] * 15 + [C.c_void_p, C.c_void_p]
    decl = re.search(r"\bint dpl_mx_conv\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(argtypes) and decl.count("int64_t") == 15
    from dipoorlet_amd.csrc import build as hipbuild
    assert any(p.endswith("mx_conv_kernels.hip") for p in hipbuild.SRC)
