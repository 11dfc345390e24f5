"""The error bounds the executor's operators are held to against tests/onnx_ref.py, per kind of operator, and the figures they were
derived from (measured on an MI355X and on the CPU) — shared by test_executor_ops_onnx.py (hand-built nodes, one operator each) and
qdq_replay.py (the nodes of a saved Q/DQ model against the session that produced it).  The derivations are in
test_executor_ops_onnx.py's docstring; nothing here is tuned to a test's result.

  exact  bit for bit against the model's result cast to fp32
  sum    (K + 2) 2^-24 sum |terms| for a K-term sum in any order of fp32 accumulation (the model supplies sum |terms| as aux['mag'])
  conv   the same on the CPU; on the device DEVICE_CONV_RATIO 2^-24 sum |x w| (the library may choose Winograd or split-K solvers)
  trans  TRANS_RATIO 2^-24 max(|ref|, 1) for what goes through library functions
"""
import numpy as np

U = 2.0 ** -24

# largest |got - ref| / (2^-24 sum |x w|) per convolution case, measured on an MI355X (MIOpen's FAST find mode, fp32)
CONV_MEASURED = {
    "conv_2d_k1": 2.779,
    "convt_2d_asym": 2.48,
    "conv_2d_sym": 2.086,
    "convt_2d_output_shape": 1.891,
    "conv_2d_s2_d2_asym": 1.794,
    "conv_3d_asym": 1.774,
    "convt_2d_valid": 1.695,
    "conv_2d_asym_nobias": 1.651,
    "conv_2d_same_lower": 1.591,
    "convt_3d_asym": 1.569,
    "conv_2d_group2": 1.553,
    "convt_2d_group3": 1.543,
    "convt_2d_same_upper": 1.492,
    "convt_2d_s2_opad": 1.485,
    "convt_2d_asym_opad": 1.426,
    "conv_2d_group3_k5x1": 1.395,
    "conv_2d_same_upper_dilated": 1.371,
    "convt_2d_output_shape_opad": 1.362,
    "convt_2d_same_lower": 1.319,
    "conv_2d_depthwise": 1.311,
    "conv_2d_same_upper": 1.294,
    "convt_2d_dilated": 1.292,
    "conv_3d_group_same_lower": 1.27,
    "conv_1d_s2_d2_asym": 1.087,
    "convt_1d_asym": 1.017,
    "conv_2d_valid": 0.87,
}
DEVICE_CONV_RATIO = 4.0 * max(list(CONV_MEASURED.values()) + [1.0])
# largest |got - ref| / (2^-24 max(|ref|, 1)) per operator, measured: (CPU, MI355X)
TRANS_MEASURED = {
    "LayerNormalization": (4.462, 6.74),
    "InstanceNormalization": (2.367, 6.318),
    "Gelu": (3.855, 1.43),
    "HardSwish": (1.601, 2.495),
    "BatchNormalization": (1.636, 2.131),
    "Log": (0.958, 1.532),
    "Pow": (0.936, 1.442),
    "Softmax": (1.305, 1.305),
    "Erf": (0.889, 1.14),
    "Sigmoid": (1.024, 1.024),
    "Sub": (0.999, 0.999),
    "Exp": (0.917, 0.975),
    "Add": (0.974, 0.974),
    "Div": (0.968, 0.968),
    "Mul": (0.948, 0.948),
    "Sqrt": (0.909, 0.909),
    "Eltwise": (0.899, 0.899),
    "Reciprocal": (0.895, 0.895),
    "HardSigmoid": (0.8, 0.8),
    "Tanh": (0.503, 0.74),
    "PRelu": (0.701, 0.701),
    "LeakyRelu": (0.499, 0.499),
}
TRANS_RATIO = 4.0 * max([v for pair in TRANS_MEASURED.values() for v in pair] + [1.0])


class Case:
    def __init__(self, id, op, inputs, attrs=None, opset=13, kind="exact", K=0, feeds=(0,), session=True, n_out=1, refuse=None):
        self.id, self.op, self.inputs, self.attrs, self.opset = id, op, inputs, dict(attrs or {}), opset
        self.kind, self.K, self.feeds, self.session, self.n_out, self.refuse = kind, K, tuple(feeds), session, n_out, refuse

    def __repr__(self):
        return self.id


def _bound(c, ref, aux, device_type):
    """The absolute error allowed per output (None: bit for bit) and the unit the error is reported in."""
    if c.kind == "exact":
        return None, None
    if c.kind == "trans":
        unit = U * np.maximum(np.abs(ref), 1.0)
        return TRANS_RATIO * unit, unit
    unit = U * aux["mag"]
    if c.kind == "conv" and device_type == "cuda":
        return DEVICE_CONV_RATIO * unit, unit
    return (c.K + 2) * unit, unit


def _check(c, got, ref, aux, device_type, what=""):
    """got against the model; returns the largest error in the case's unit (0.0 for an exact case)."""
    assert len(got) == len(ref), (c.id, len(got), len(ref))
    worst = 0.0
    for g, r in zip(got, ref):
        assert tuple(g.shape) == tuple(r.shape), f"{c.id}{what}: shape {g.shape}, defined {r.shape}"
        bound, unit = _bound(c, r, aux, device_type)
        if bound is None:
            want = r.astype(g.dtype) if r.dtype != g.dtype else r
            assert g.dtype == (np.float32 if r.dtype == np.float64 else r.dtype), (c.id, g.dtype, r.dtype)
            assert np.array_equal(g, want, equal_nan=g.dtype.kind == "f"), f"{c.id}{what}: not the defined values, bit for bit"
            continue
        assert g.dtype == np.float32, (c.id, g.dtype)
        err = np.abs(g.astype(np.float64) - r)
        ratio = float(np.divide(err, unit, out=np.zeros_like(err), where=unit > 0).max()) if err.size else 0.0     # (unit 0: err 0, below)
        worst = max(worst, ratio)
        print(f"{c.id}{what} [{device_type}]: largest error {ratio:.3f} units, allowed {float(np.max(bound[unit > 0] / unit[unit > 0])):.1f}")
        assert np.isfinite(g).all() and (err <= bound).all(), f"{c.id}{what}: {ratio:.3f} units off the definition"
    return worst


def _one_tap_condition(c, aux, device_type):
    """The bound must not be able to hide a dropped kernel position or pad row: below 1 % of the smallest product in each output."""
    ratio = DEVICE_CONV_RATIO if device_type == "cuda" else c.K + 2
    tap = aux["min_tap"]
    seen = np.isfinite(tap)                 # (an output no product reaches — output_padding — has nothing to lose)
    assert seen.any() and (ratio * U * aux["mag"][seen] < 0.01 * tap[seen]).all(), \
        (c.id, float((ratio * U * aux["mag"][seen] / tap[seen]).max()))
