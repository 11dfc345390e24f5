"""CPU: the two translations of a quantize.QDQNode side by side, without a device.  The in-process form is the fused FakeQuant
node, whose parameters are the node's fields (scale, the zero point as stored, saturation(), axis): interpreted here by the models
that the kernels are held to (oracle.np_oracle.fake_quant_qdq, fp8_model.fake_quant_fp8).  The deployed form is the file that
graph.to_model / insert_qnodes_purely write: saved, reloaded and interpreted by tests/onnx_ref.py's QuantizeLinear /
DequantizeLinear (written from the operator text).  Over the same activations — an fp64 forward of the network on images that leave
the calibrated ranges — every pair's output must agree bit for bit, on all nine platforms and both layouts of the Gemm weight."""
import types

import numpy as np
import pytest

import fp8_model
import qdq_replay as Q
from dipoorlet_amd.platform_settings import platform_setting_table
from dipoorlet_amd.quantize import FP8_E4M3, get_qnode_by_param, quant_graph
from oracle import np_oracle as O


def _copy(clip):
    return {k: [np.copy(v[0]), np.copy(v[1])] for k, v in clip.items()}


@pytest.fixture(scope="module", params=[1, 0], ids=["transB1", "transB0"])
def net(request):
    """(graph, ranges, the replay activations): built once per layout, never written to."""
    g = Q.build_conv_net(request.param)
    calib = Q.reference_forward(g, Q.images((3, Q.IMG, Q.IMG), Q.N_CALIB, 4))
    act, wt = Q.host_ranges(g, calib)
    acts = Q.reference_forward(g, Q.images((3, Q.IMG, Q.IMG), Q.N_REPLAY, 5, Q.REPLAY_SCALE))
    for a in acts.values():
        a.setflags(write=False)
    return g, {**act, **wt}, acts


def _fake_quant_by_the_models(q, x):
    """The FakeQuant node of `q` on x, from the node's fields, by the models the kernels are held to."""
    axis = q.axis if q.scale.size > 1 else None
    if q.fmt == FP8_E4M3:
        return fp8_model.fake_quant_fp8(x, q.scale, axis)
    assert q.fmt == "Linear" and q.saturation() == ((-128, 127) if q.symmetric else (0, 255))
    assert np.array_equal(q.zero_point_as_stored(), q.zero_point.astype(np.int64) & 0xFF if not q.symmetric else q.zero_point)
    return O.fake_quant_qdq(x, q.scale, q.zero_point, axis=axis, signed=q.symmetric)


@pytest.mark.parametrize("deploy", list(platform_setting_table))
def test_saved_file_and_fake_quant_graph_define_the_same_pairs(net, deploy, tmp_path):
    g, clip, acts = net
    args = types.SimpleNamespace(deploy=deploy, skip_layers=[], mx=None)
    gq, _ = quant_graph(g, _copy(clip), args)
    gq.output_dir = str(tmp_path)
    path = gq.save_onnx_model("quant_model")
    # the FakeQuant graph, interpreted directly
    session = dict(acts)
    for n in gq.graph.node:
        if n.op_type == "FakeQuant":
            q = gq._qdq[n.name]
            x = gq.initializer[n.input[0]] if n.input[0] in gq.initializer else acts[n.input[0]]
            session[n.output[0]] = _fake_quant_by_the_models(q, x)
    assert platform_setting_table[deploy]["quantize_network_output"] == ("output_dq" in session)
    # the file, interpreted by the ONNX definitions: the same tensors under the names the FILE uses
    results = Q.replay(path, session.__getitem__)
    pairs = [r for r in results if r.node.op_type == "DequantizeLinear"]
    assert len(pairs) == sum(n.op_type == "FakeQuant" for n in gq.graph.node) >= 6
    for r in pairs:
        assert Q.same_bits(r.y[0], session[r.node.output[0]]), f"{deploy}: {r.node.output[0]} of the file is not the FakeQuant node's"
    # every other node of the file reads what the FakeQuant graph's node of that name reads
    by_name = {n.name: n for n in gq.graph.node}
    for r in results:
        if r.node.op_type != "DequantizeLinear":
            assert list(r.node.input) == list(by_name[r.node.name].input), r.id
    # both ends of the grids were reached, by activations: the zero-point and saturation arithmetic was exercised
    n, lo, hi = Q.saturation_census(results)
    print(f"{deploy}: {len(pairs)} pairs, {n} of them activations; {lo} reach the lowest code, {hi} the highest")
    assert lo >= 1 and hi >= 1
    # a per-channel weight pair of a ConvTranspose runs along axis 1, of everything else along axis 0 (atlas leaves ConvTranspose alone)
    if platform_setting_table[deploy]["qw_params"].get("per_channel"):
        axes = {r.source: r.node.attrs.get("axis") for r in pairs if r.weight and np.asarray(r.inputs[r.node.input[1]]).size > 1}
        assert axes.pop("ct.weight", 1) == 1 and axes == {"c1.weight": 0, "c2.weight": 0, "fc.weight": 0}, axes


def test_asymmetric_zero_points_above_127_are_in_the_files(net, tmp_path):
    """The zero points the int8 storage wraps (quantize._int8_wrap) must come back from the file as the uint8 values."""
    g, clip, acts = net
    gq, _ = quant_graph(g, _copy(clip), types.SimpleNamespace(deploy="snpe", skip_layers=[], mx=None))
    gq.output_dir = str(tmp_path)
    from dipoorlet_amd import onnx_io
    m = onnx_io.load_model(gq.save_onnx_model("q"))
    zps = {k: v for k, v in m.initializers.items() if k.endswith("_zero_point")}
    assert all(v.dtype == np.uint8 for v in zps.values()) and max(int(v.max()) for v in zps.values()) > 127
    for q in gq._qdq.values():
        assert np.array_equal(np.asarray(zps[q.zero_point_name]).reshape(-1), q.zero_point_as_stored())


def test_channel_scales_that_do_not_match_their_axis_are_refused(net, tmp_path):
    """Ranges taken along axis 0 of the ConvTranspose weight [8, 6, 2, 2] (8 of them) for a pair that runs along axis 1 (6 slices):
    quant_graph refuses by the tensor's name; so does save_onnx_model of a graph that was given such a node by hand."""
    g, clip, _ = net
    bad = _copy(clip)
    w = np.asarray(g.get_initializer("ct.weight")).reshape(8, -1)
    bad["ct.weight"] = [w.min(-1), w.max(-1)]
    for deploy in ("trt", "ocp_fp8"):
        with pytest.raises(ValueError, match=r"ct\.weight.*8 channel scales for axis 1"):
            quant_graph(g, _copy(bad), types.SimpleNamespace(deploy=deploy, skip_layers=[], mx=None))
    gq, _ = quant_graph(g, _copy(clip), types.SimpleNamespace(deploy="trt", skip_layers=[], mx=None))
    q, _, _ = get_qnode_by_param(platform_setting_table["trt"]["qw_params"], "ct.weight", [8, 6, 2, 2], [w.min(-1), w.max(-1)], True)
    gq._qdq[q.q_name] = q
    gq.output_dir = str(tmp_path)
    with pytest.raises(ValueError, match=r"ct\.weight.*8 channel scales for axis 1"):
        gq.save_onnx_model("bad")
    # one scale for the whole tensor stays legal on a per-channel platform's node, and the right number passes
    quant_graph(g, _copy(clip), types.SimpleNamespace(deploy="trt", skip_layers=[], mx=None))
