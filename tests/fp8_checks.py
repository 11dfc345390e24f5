"""What a saved Q/DQ model of the `ocp_fp8` platform must look like — shared by tests/test_fp8_model.py (a hand-made graph) and
tests/test_fp8_gpu.py (the CLI's quant_model.onnx)."""
import numpy as np


def check_saved_fp8_model(path, n_pairs_at_least, per_channel_axis):
    """A saved Q/DQ model of the ocp_fp8 platform: opset >= 19, every pair's zero point a FLOAT8E4M3FN tensor of zero bytes with
    its scale's element count, per-channel pairs carrying their axis -> the number of pairs.  (Shared with the GPU CLI test.)"""
    from dipoorlet_amd import onnx_io
    m = onnx_io.load_model(str(path))
    assert m.opset[""] >= 19 and m.ir_version >= 9
    qs = [n for n in m.nodes if n.op_type == "QuantizeLinear"]
    dqs = {n.name: n for n in m.nodes if n.op_type == "DequantizeLinear"}
    assert len(qs) == len(dqs) >= n_pairs_at_least
    for n in qs:
        t = n.input[0]
        dq = dqs[t + "_DequantizeLinear"]
        assert n.input[1:] == [t + "_scale", t + "_zero_point"] == dq.input[1:] and dq.input[0] == n.output[0] == t + "_q"
        scale, zp = m.initializers[t + "_scale"], m.initializers[t + "_zero_point"]
        assert isinstance(zp, onnx_io.Float8E4M3FNBytes) and zp.dtype == np.uint8, t
        assert scale.dtype == np.float32 and zp.shape == scale.shape and not zp.any(), t
        if scale.size > 1:
            assert n.attrs["axis"] == dq.attrs["axis"] == per_channel_axis(t), t
        else:
            assert "axis" not in n.attrs and scale.shape == ()
    return len(qs)
