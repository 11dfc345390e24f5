"""CPU: the `Float8E4M3FN` quantisation type below the kernel — the numpy definition (tests/fp8_model.py) against torch's CPU cast,
the scale derivation, the CLI's argument check, the saved Q/DQ model, the emitter and the binding."""
import json
import types

import numpy as np
import pytest
import torch

import fp8_model as M
from fp8_checks import check_saved_fp8_model


# ------------------------------------------------------------------------------------------------ 1. the model
def _torch_cast(v):
    return torch.from_numpy(v).to(torch.float8_e4m3fn).to(torch.float32).numpy()


def test_codes_are_the_formats_own():
    """The point set is built from the encoding: 127 finite non-negative codes, read back by torch bit for bit."""
    codes = M.e4m3_codes()
    assert codes.size == 127 and codes[0] == 0 and codes[1] == 2.0 ** -9 and codes[8] == 2.0 ** -6 and codes[-1] == 448
    want = torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert np.array_equal(codes, want)
    assert np.array_equal(M.e4m3_round(codes), codes) and np.array_equal(M.e4m3_round(-codes), -codes)


def test_model_against_torch_cpu_cast():
    """Every code, every tie between two codes, the fp32 neighbours of both, 464 and its lower neighbour, both signs, and 2^20
    log-uniform values: equal values and equal sign bits (the sign of zero included), no exclusions.  torch's cast does not
    saturate (464 -> 448, above -> NaN), so the comparison ends at |v| = 464."""
    rng = np.random.default_rng(17)
    mag = np.exp2(rng.uniform(-14.0, np.log2(464.0), 1 << 20)).astype(np.float32)
    rand = np.minimum(mag, np.float32(464.0)) * rng.choice(np.array([-1, 1], np.float32), mag.size)
    v = np.concatenate([M.boundary_points(), rand])
    assert np.abs(v).max() == 464 and v.size > (1 << 20) + 1500
    got, want = M.e4m3_round(v), _torch_cast(v)
    assert not np.isnan(want).any()
    bad = np.flatnonzero((got != want) | (np.signbit(got) != np.signbit(want)))
    assert bad.size == 0, (bad.size, v[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_ties_go_to_even_in_the_subnormal_range_too():
    step = 2.0 ** -9
    v = np.array([0.5 * step, 1.5 * step, 2.5 * step, 7.5 * step, 17.0, 19.0, 464.0, -0.5 * step], np.float32)
    want = np.array([0.0, 2 * step, 2 * step, 8 * step, 16.0, 20.0, 448.0, -0.0], np.float32)
    got = M.e4m3_round(v)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


def test_saturation_infinities_and_nan():
    inf = np.float32(np.inf)
    v = np.array([np.nextafter(np.float32(464), inf), 480.0, 1e9, inf, -500.0, -1e9, -inf, 3.4e38], np.float32)
    assert np.array_equal(M.e4m3_round(v), np.array([448, 448, 448, 448, -448, -448, -448, 448], np.float32))
    assert np.isnan(M.e4m3_round(np.array([np.nan, -np.nan], np.float32))).all()
    y = M.fake_quant_fp8(np.array([np.nan, np.inf, -np.inf, 1.0], np.float32), [0.5])
    assert np.isnan(y[0]) and np.array_equal(y[1:], np.array([224.0, -224.0, 1.0], np.float32))


def test_fake_quant_is_two_single_fp32_operations_and_follows_the_axis():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 5)).astype(np.float32) * 4
    s = np.array([0.0123, 1.0, 3e-3], np.float32)
    y = M.fake_quant_fp8(x, s, axis=1)
    for c in range(3):
        q = M.e4m3_round((x[:, c] / s[c]).astype(np.float32))
        assert np.array_equal(y[:, c], (q * s[c]).astype(np.float32))
    assert np.array_equal(M.fake_quant_fp8(x, s[:1]), M.fake_quant_fp8(x, np.full(3, s[0], np.float32), axis=1))


# ------------------------------------------------------------------------------------------------ 2. scales
def test_get_qnode_by_param_derives_clip_over_448():
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.quantize import get_qnode_by_param
    plat = platform_setting_table["ocp_fp8"]
    assert plat["quant_nodes"] == ["Conv", "Gemm", "ConvTranspose", "MatMul"]
    assert plat["qw_params"] == {"bit_width": 8, "type": "Float8E4M3FN", "symmetric": True, "per_channel": True}
    assert plat["qi_params"] == {"bit_width": 8, "type": "Float8E4M3FN", "symmetric": True}
    q, lo, hi = get_qnode_by_param(plat["qi_params"], "t", [1, 4], [-3.5, 2.0])
    assert (lo, hi) == (-448, 448) and q.saturation() == (-448, 448) and q.zp_dtype == "float8e4m3fn" and q.axis is None
    assert q.scale.dtype == np.float32 and q.scale.tolist() == [float(np.float32(3.5 / 448))]
    assert q.zero_point.tolist() == [0] and q.output == "t_dq"
    rng = [np.array([-1.0, 0.0, -0.25]), np.array([3.0, 0.0, 0.125])]
    q, lo, hi = get_qnode_by_param(plat["qw_params"], "w", [3, 2], rng)
    assert (lo, hi) == (-448, 448) and q.axis == 0 and q.per_channel
    assert q.scale.tolist() == [float(np.float32(3.0 / 448)), 1.0, float(np.float32(0.25 / 448))]      # an all-zero channel: 1
    assert rng[0].tolist() == [-1.0, 0.0, -0.25]                                                      # per channel: left alone
    q, _, _ = get_qnode_by_param(plat["qw_params"], "w", [3, 2], rng, need_transpose=True)
    assert q.axis == 1
    # a per-tensor parameter set collapses per-channel ranges IN PLACE, as the Linear branch does
    q, _, _ = get_qnode_by_param(plat["qi_params"], "w", [3, 2], rng)
    assert q.scale.tolist() == [float(np.float32(3.0 / 448))] and rng[0] == -1.0 and rng[1] == 3.0
    q, _, _ = get_qnode_by_param(plat["qi_params"], "z", [1], [0.0, 0.0])
    assert q.scale.tolist() == [1.0]


def test_linear_nodes_are_what_they_were():
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.quantize import QDQNode, get_qnode_by_param
    q, lo, hi = get_qnode_by_param(platform_setting_table["trt"]["qi_params"], "t", [1], [-1.0, 2.0])
    assert q.fmt == "Linear" and q.zp_dtype == "int8" and q.saturation() == (-128, 127) and (lo, hi) == ([-127], [127])
    assert QDQNode("t", [1], [1.0], [0], False, False, False).zp_dtype == "uint8"
    assert get_qnode_by_param({"type": "Log"}, "t", [1], [-1.0, 1.0]) == (None, None, None)


# ------------------------------------------------------------------------------------------------ 3. CLI
def _parse(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", *extra])


@pytest.mark.parametrize("flags", [["-A", "mse"], ["-A", "kl"], ["-A", "hist", "--adaround"], ["-A", "hist", "--brecq"],
                                   ["-A", "minmax", "--sparse"]])
def test_cli_refuses_what_assumes_an_integer_grid(flags):
    from dipoorlet_amd.__main__ import check_args
    args = _parse("-D", "ocp_fp8", *flags)
    assert args.deploy == "ocp_fp8"
    with pytest.raises(ValueError) as e:
        check_args(args)
    msg = str(e.value)
    assert flags[-1] in msg and "-A minmax" in msg and "-A hist" in msg and "--bc" in msg


@pytest.mark.parametrize("flags", [["-A", "minmax"], ["-A", "hist"], ["-A", "hist", "--bc", "--we", "--update_bn"]])
def test_cli_passes_what_reaches_the_grid_through_fake_quant_nodes(flags):
    from dipoorlet_amd.__main__ import check_args
    check_args(_parse("-D", "ocp_fp8", *flags))


def test_cli_check_leaves_integer_platforms_alone():
    from dipoorlet_amd.__main__ import check_args
    check_args(_parse("-D", "trt", "-A", "mse", "--adaround", "--brecq", "--sparse"))
    check_args(_parse("-D", "snpe", "-A", "kl"))


# ------------------------------------------------------------------------------------------------ 4. save and reload
def _three_node_graph():
    from dipoorlet_amd.models import _B
    g = _B(5)
    x = g.conv("input", 3, 4, 3, 1, 1, "c1")
    x = g.node("Relu", [x], out="r1_out")
    x = g.conv(x, 4, 2, 1, 1, 0, "c2")
    return g.finish("input", [1, 3, 6, 6], x)


def test_save_and_reload_a_graph_with_fp8_pairs(tmp_path):
    from dipoorlet_amd import onnx_io
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.quantize import get_qnode_by_param
    g = _three_node_graph()
    g.output_dir = str(tmp_path)
    before = g.save_onnx_model("plain")
    plat = platform_setting_table["ocp_fp8"]
    c1 = next(n for n in g.graph.node if n.output[0] == "c1_out")
    w = g.get_initializer("c1.weight").reshape(4, -1)
    qa, _, _ = get_qnode_by_param(plat["qi_params"], "input", g.get_tensor_shape("input"), [-2.0, 3.0])
    qw, _, _ = get_qnode_by_param(plat["qw_params"], "c1.weight", [4, 3, 3, 3], [w.min(1), w.max(1)])
    for q, slot in ((qa, 0), (qw, 1)):
        c1.input[slot] = q.output
        g.insert_qnodes_purely(q_nodes=q, node=c1)
    g.update_model()
    path = g.save_onnx_model("fp8")
    assert check_saved_fp8_model(path, 2, lambda t: 0) == 2
    m = onnx_io.load_model(path)
    assert m.initializers["input_zero_point"].shape == () and m.initializers["c1.weight_zero_point"].shape == (4,)
    assert np.array_equal(m.initializers["c1.weight_scale"], qw.scale) and m.initializers["input_scale"] == qa.scale[0]
    # the bytes on disk: data type 17, one raw 0x00 byte per element
    raw = open(path, "rb").read()
    zp_proto = onnx_io._enc_tensor("c1.weight_zero_point", m.initializers["c1.weight_zero_point"])
    assert zp_proto == b"\x08\x04\x10\x11" + b"\x42\x14c1.weight_zero_point" + b"\x4a\x04\x00\x00\x00\x00" and zp_proto in raw
    # written again from the reloaded model: the same file; and a graph without FP8 nodes keeps its opset and its bytes
    again = str(tmp_path / "again.onnx")
    onnx_io.save_model(m, again)
    assert open(again, "rb").read() == raw
    plain = onnx_io.load_model(before)
    assert plain.opset[""] == 13 and plain.ir_version == 8
    g2 = _three_node_graph()
    g2.output_dir = str(tmp_path)
    assert open(g2.save_onnx_model("plain2"), "rb").read() == open(before, "rb").read()


# ------------------------------------------------------------------------------------------------ 5. emitter
def test_emitter_writes_the_scales_get_qnode_by_param_derives(tmp_path):
    from dipoorlet_amd.deploy import to_deploy
    act = {"input": [-3.5, 2.0], "c1_out": [0.0, 0.0], "r1_out": [0.0, 7.0]}
    wt = {"c1.weight": [[-1.0, -2.0], [1.0, 0.5]]}
    args = types.SimpleNamespace(deploy="ocp_fp8", output_dir=str(tmp_path))
    to_deploy(None, act, wt, args)
    want = {"format": "float8e4m3fn", "scale": {"input": float(np.float32(3.5 / 448)), "c1_out": 1.0,
                                                 "r1_out": float(np.float32(7.0 / 448))}}
    assert open(tmp_path / "ocp_fp8_scales.json").read() == json.dumps(want, indent=4)
    assert act["input"] == [-3.5, 2.0]


# ------------------------------------------------------------------------------------------------ 6. ABI
def test_binding_declares_the_entry_points():
    import ctypes as C

    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 24
    i32, i64, p = C.c_int32, C.c_int64, C.c_void_p
    assert _hip.SIGNATURES["dpl_fake_quant_fp8"] == (C.c_int, [i32, p, p, p, i64, p, i64, i64, p])
    assert _hip.SIGNATURES["dpl_fake_quant_fp8_items"] == _hip.SIGNATURES["dpl_fake_quant_items"]
