"""Per-backend quantisation settings (data only).

Same keys and values as the reference table (dipoorlet/platform_settings.py:1-184) because the
calibration hot path reads them verbatim: `'dynamic_sym' in qi_params` decides OCTAV's `unsigned`
factor (forward_net.py:319) and qi/qw params feed scale / zero-point derivation (quantize.py:111-194).
Expressed through a small builder instead of eight literal dicts.

`ocp_fp8` is this project's own entry (the reference has no floating-point grid): static per-tensor / per-channel scales for
OCP FP8 E4M3, type "Float8E4M3FN" — `bit_width` stays 8, the width of the format (quantize.get_qnode_by_param).
`mx_setting_table` (`--mx`, with `-D ocp_fp8` only) is no platform: the OCP Microscaling parameter sets that replace the platform's
on both operands of MatMul and Gemm — blocks of 32 along the reduction axis with a shared power-of-two scale, no static scale.
"""

LAYER_HAS_WEIGHT = ["Conv", "Gemm", "ConvTranspose", "PRelu", "BatchNormalization"]

_BASIC = ["Relu", "Eltwise", "MaxPool", "Conv", "Gemm", "ConvTranspose", "PRelu", "AveragePool", "Concat",
          "Split", "Add", "Mul", "Abs", "Reciprocal", "Sigmoid"]


def _lin(symmetric, **extra):
    d = {"bit_width": 8, "type": "Linear", "symmetric": symmetric}
    d.update(extra)
    return d


def _fp8(**extra):
    d = {"bit_width": 8, "type": "Float8E4M3FN", "symmetric": True}
    d.update(extra)
    return d


def _platform(quant_nodes, qw, qi, net_out=False, deploy_weight=False, exclude=True):
    d = {"quant_nodes": list(quant_nodes), "qw_params": qw, "qi_params": qi,
         "quantize_network_output": net_out, "deploy_weight": deploy_weight}
    if exclude:
        d["deploy_exclude_layers"] = []
    return d


platform_setting_table = {
    "trt": _platform(["Relu", "MaxPool", "Conv", "Gemm", "ConvTranspose", "PRelu", "AveragePool", "Add",
                      "Sigmoid"], _lin(True, per_channel=True), _lin(True)),
    "stpu": _platform(_BASIC + ["Clip", "HardSigmoid"], _lin(True, per_channel=False), _lin(True),
                      deploy_weight=True),
    "magicmind": _platform(["Gemm", "Conv", "ConvTranspose", "MatMul"],
                           _lin(False, log_scale=False, per_channel=True), _lin(False, log_scale=False)),
    "rv": _platform(_BASIC, _lin(False, per_channel=False), _lin(False), net_out=True, deploy_weight=True),
    "atlas": _platform(["Conv", "Gemm", "AveragePool"], _lin(True, per_channel=True), _lin(False),
                       exclude=False),
    "snpe": _platform(_BASIC + ["Sigmoid"], _lin(False, per_channel=False), _lin(False), net_out=True),
    "ti": _platform(_BASIC, _lin(True, per_channel=False, log_scale=False),
                    _lin(True, dynamic_sym=True, log_scale=True)),
    "imx": _platform(_BASIC, _lin(True, per_channel=True, log_scale=True), _lin(True, log_scale=True),
                     net_out=True, deploy_weight=True),
    "ocp_fp8": _platform(["Conv", "Gemm", "ConvTranspose", "MatMul"], _fp8(per_channel=True), _fp8()),
}

mx_setting_table = {
    "mxfp8": {"bit_width": 8, "type": "MXFP8E4M3", "block_size": 32},
    "mxfp4": {"bit_width": 4, "type": "MXFP4E2M1", "block_size": 32},
}
# The two OCP MXFP6 formats of `--mx` (tests/mx_fp6_model.py), beside the table above: everything --mx offers but --mx_gptq and
# --mx_mixed, which are held to the two formats of mx_setting_table.
mx_fp6_setting_table = {
    "mxfp6_e2m3": {"bit_width": 6, "type": "MXFP6E2M3", "block_size": 32},
    "mxfp6_e3m2": {"bit_width": 6, "type": "MXFP6E3M2", "block_size": 32},
}
MX_CHOICES = tuple(mx_setting_table) + tuple(mx_fp6_setting_table)      # what --mx takes


def mx_setting(name):
    """The parameter set of `--mx name`: the one way from a format's name to its set, whichever table holds it."""
    return mx_setting_table[name] if name in mx_setting_table else mx_fp6_setting_table[name]
