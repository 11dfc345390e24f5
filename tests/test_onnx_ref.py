"""CPU: tests/onnx_ref.py — the numpy fp64 model of the ONNX operator definitions that test_executor_ops_onnx.py holds the
executor's op table to — against values worked out by hand from the definitions (the arithmetic is in the comments)."""
import numpy as np
import pytest

import onnx_ref
from onnx_ref import REF

X22 = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32).reshape(1, 1, 2, 2)


def _resize(x, attrs, sizes=None, scales=None, opset=13):
    inputs = [x, None, None if scales is None else np.asarray(scales, np.float32), None if sizes is None else np.asarray(sizes, np.int64)]
    return REF["Resize"](inputs, attrs, opset)[0]


@pytest.mark.parametrize("coord,row0,at11,at21", [
    # x_orig(o) = (o + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25, clamped to [0, 1]: weights 0, 0.25, 0.75, 1 on each axis.
    # row 0 (weight 0 down): 1 + t = 1, 1.25, 1.75, 2.  (1, 1): top 1.25, bottom 3.25, 0.25 down: 1.25 + 0.25 * 2 = 1.75.
    # (2, 1): 0.75 down: 1.25 + 0.75 * 2 = 2.75
    ("half_pixel", [1.0, 1.25, 1.75, 2.0], 1.75, 2.75),
    ("pytorch_half_pixel", [1.0, 1.25, 1.75, 2.0], 1.75, 2.75),            # (out > 1: the same coordinates)
    # x_orig(o) = o * (2 - 1) / (4 - 1) = 0, 1/3, 2/3, 1.  row 0: 1, 4/3, 5/3, 2.  (1, 1): 1 + 1/3 * 1 + 1/3 * 2 = 2.
    # (2, 1): 1 + 1/3 * 1 + 2/3 * 2 = 8/3
    ("align_corners", [1.0, 4 / 3, 5 / 3, 2.0], 2.0, 8 / 3),
    # x_orig(o) = o / 2 = 0, 0.5, 1, 1.5 -> 1 (clamped).  row 0: 1, 1.5, 2, 2.  (1, 1): 1 + 0.5 * 1 + 0.5 * 2 = 2.5.
    # (2, 1): weight 1 down: 3 + 0.5 = 3.5
    ("asymmetric", [1.0, 1.5, 2.0, 2.0], 2.5, 3.5),
])
def test_linear_resize_2x2_to_4x4_per_coordinate_mode(coord, row0, at11, at21):
    y = _resize(X22, {"mode": "linear", "coordinate_transformation_mode": coord}, sizes=[1, 1, 4, 4])
    assert y.shape == (1, 1, 4, 4)
    np.testing.assert_allclose(y[0, 0, 0], row0, rtol=0, atol=1e-15)
    np.testing.assert_allclose([y[0, 0, 1, 1], y[0, 0, 2, 1], y[0, 0, 3, 3]], [at11, at21, 4.0], rtol=0, atol=1e-15)
    # the same by scales = 2: out = floor(2 * 2), the coordinates divide by the given scale
    np.testing.assert_array_equal(_resize(X22, {"mode": "linear", "coordinate_transformation_mode": coord}, scales=[1, 1, 2, 2]), y)


def test_resize_to_one_pixel_pytorch_half_pixel_reads_the_origin():
    # out = 1: pytorch_half_pixel -> x_orig = 0 on both axes -> x[0, 0] = 1; half_pixel -> (0 + 0.5) / 0.5 - 0.5 = 0.5 on both
    # axes -> the mean of the four = 2.5
    assert _resize(X22, {"mode": "linear", "coordinate_transformation_mode": "pytorch_half_pixel"}, sizes=[1, 1, 1, 1]).item() == 1.0
    assert _resize(X22, {"mode": "linear", "coordinate_transformation_mode": "half_pixel"}, sizes=[1, 1, 1, 1]).item() == 2.5


@pytest.mark.parametrize("coord,nearest,index", [
    # half_pixel, scale 8 / 5: x_orig = (o + 0.5) / 1.6 - 0.5 = -0.1875 0.4375 1.0625 1.6875 2.3125 2.9375 3.5625 4.1875
    ("half_pixel", "round_prefer_floor", [0, 0, 1, 2, 2, 3, 4, 4]),     # ceil(x - 0.5): o = 2: ceil(0.5625) = 1; o = 3: ceil(1.1875) = 2
    ("half_pixel", "round_prefer_ceil", [0, 0, 1, 2, 2, 3, 4, 4]),      # floor(x + 0.5): o = 2: floor(1.5625) = 1; o = 6: floor(4.0625) = 4
    ("half_pixel", "floor", [0, 0, 1, 1, 2, 2, 3, 4]),                  # o = 0: floor(-0.1875) = -1 -> clamped to 0; o = 3: floor(1.6875) = 1
    ("half_pixel", "ceil", [0, 1, 2, 2, 3, 3, 4, 4]),                   # o = 1: ceil(0.4375) = 1; o = 7: ceil(4.1875) = 5 -> clamped to 4
    # asymmetric: x_orig = o / 1.6 = 0 0.625 1.25 1.875 2.5 3.125 3.75 4.375 — o = 4 is a tie
    ("asymmetric", "round_prefer_floor", [0, 1, 1, 2, 2, 3, 4, 4]),     # o = 4: ceil(2.5 - 0.5) = 2 (the tie goes down); o = 1: ceil(0.125) = 1
    ("asymmetric", "round_prefer_ceil", [0, 1, 1, 2, 3, 3, 4, 4]),      # o = 4: floor(2.5 + 0.5) = 3 (the tie goes up); o = 6: floor(4.25) = 4
    ("asymmetric", "floor", [0, 0, 1, 1, 2, 3, 3, 4]),                  # o = 1: floor(0.625) = 0; o = 5: floor(3.125) = 3
    ("asymmetric", "ceil", [0, 1, 2, 2, 3, 4, 4, 4]),                   # o = 2: ceil(1.25) = 2; o = 7: ceil(4.375) = 5 -> clamped to 4
])
def test_nearest_resize_5_to_8_under_each_nearest_mode(coord, nearest, index):
    x = np.arange(10, 15, dtype=np.float32).reshape(1, 1, 5)
    y = _resize(x, {"mode": "nearest", "coordinate_transformation_mode": coord, "nearest_mode": nearest}, sizes=[1, 1, 8])
    np.testing.assert_array_equal(y.reshape(-1) - 10, index)


def test_resize_defaults_by_opset():
    x = np.arange(10, 15, dtype=np.float32).reshape(1, 1, 5)
    # opset 11+, no attributes: half_pixel / round_prefer_floor (the first row of the table above)
    np.testing.assert_array_equal(_resize(x, {}, sizes=[1, 1, 8]).reshape(-1) - 10, [0, 0, 1, 2, 2, 3, 4, 4])
    # Resize-10 and Upsample: (X, scales), x_orig = o / 1.6, floor — out = floor(5 * 1.6) = 8 (fp32 1.6 is a little above 1.6)
    for op, opset in (("Resize", 10), ("Upsample", 9)):
        y = REF[op]([x, np.array([1, 1, 1.6], np.float32)], {"mode": "nearest"}, opset)[0]
        np.testing.assert_array_equal(y.reshape(-1) - 10, [0, 0, 1, 1, 2, 3, 3, 4])
        # linear: x_orig(1) = 1 / 1.6 = 0.625 -> 10.625; x_orig(7) = 4.375 -> clamped to 4 -> 14
        y = REF[op]([x, np.array([1, 1, 1.6], np.float32)], {"mode": "linear"}, opset)[0].reshape(-1)
        np.testing.assert_allclose([y[1], y[7]], [10.625, 14.0], rtol=0, atol=1e-6)


def test_conv_1d_asymmetric_pads():
    x = np.array([1, 2, 3, 4], np.float32).reshape(1, 1, 4)
    w = np.array([1, 10, 100], np.float32).reshape(1, 1, 3)
    # pads [2, 0]: the taps read 0 0 1 2 3 4.  y[0] = 0 + 0 + 1 * 100 = 100; y[1] = 0 + 1 * 10 + 2 * 100 = 210;
    # y[2] = 1 + 20 + 300 = 321; y[3] = 2 + 30 + 400 = 432
    y, aux = REF["Conv"]([x, w], {"pads": [2, 0]}, 13)
    np.testing.assert_array_equal(y.reshape(-1), [100, 210, 321, 432])
    np.testing.assert_array_equal(aux["mag"].reshape(-1), [100, 210, 321, 432])
    np.testing.assert_array_equal(aux["min_tap"].reshape(-1), [100, 10, 1, 2])      # the smallest product that reaches each output
    # pads [0, 2]: 1 2 3 4 0 0.  y[2] = 3 + 40 + 0 = 43; y[3] = 4
    np.testing.assert_array_equal(REF["Conv"]([x, w], {"pads": [0, 2]}, 13)[0].reshape(-1), [321, 432, 43, 4])
    # auto_pad on a size where total is odd: in 4, k 3, stride 2: out = 2, total = (2 - 1) * 2 + 3 - 4 = 1.
    # SAME_UPPER: begin 0, end 1: windows 1 2 3 | 3 4 0 -> 321, 43.  SAME_LOWER: begin 1: 0 1 2 | 2 3 4 -> 210, 432
    np.testing.assert_array_equal(REF["Conv"]([x, w], {"auto_pad": "SAME_UPPER", "strides": [2]}, 13)[0].reshape(-1), [321, 43])
    np.testing.assert_array_equal(REF["Conv"]([x, w], {"auto_pad": "SAME_LOWER", "strides": [2]}, 13)[0].reshape(-1), [210, 432])


def test_conv_transpose_1d_asymmetric_pads_output_shape_and_auto_pad():
    x = np.array([1, 2, 3], np.float32).reshape(1, 1, 3)
    w = np.array([1, 10, 100], np.float32).reshape(1, 1, 3)
    # stride 2: input cell i lands on 2 i + t.  full length 2 * 2 + 2 + 1 = 7: 1, 10, 100 + 2, 20, 200 + 3, 30, 300
    full = [1, 10, 102, 20, 203, 30, 300]
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2]}, 13)[0].reshape(-1), full)
    # pads [1, 0] crop one in front; [0, 1] one behind
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "pads": [1, 0]}, 13)[0].reshape(-1), full[1:])
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "pads": [0, 1]}, 13)[0].reshape(-1), full[:-1])
    # output_shape 6 = in * stride: total = 7 - 6 = 1.  SAME_UPPER: begin 1 // 2 = 0, end 1; anything else: begin 1 - 0 = 1, end 0
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "auto_pad": "SAME_UPPER"}, 13)[0].reshape(-1), full[:-1])
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "auto_pad": "SAME_LOWER"}, 13)[0].reshape(-1), full[1:])
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "output_shape": [6]}, 13)[0].reshape(-1), full[1:])
    # output_padding 1 lengthens the full output by a zero: output_shape 6 then has total 2: one cropped on each side
    y = REF["ConvTranspose"]([x, w], {"strides": [2], "output_padding": [1], "output_shape": [6]}, 13)[0]
    np.testing.assert_array_equal(y.reshape(-1), full[1:])


def test_ceil_mode_last_window_kept_and_dropped():
    x5 = np.arange(1, 6, dtype=np.float32).reshape(1, 1, 5)
    # in 5, k 2, stride 2, no pads: ceil((5 - 2) / 2) + 1 = 3; the last window starts at 4 < 5: kept, it holds cell 4 alone
    attrs = {"kernel_shape": [2], "strides": [2], "ceil_mode": 1}
    np.testing.assert_array_equal(REF["MaxPool"]([x5], attrs, 13)[0].reshape(-1), [2, 4, 5])
    np.testing.assert_array_equal(REF["MaxPool"]([x5], dict(attrs, ceil_mode=0), 13)[0].reshape(-1), [2, 4])
    # in 3, pads [1, 1], k 2, stride 2: ceil((5 - 2) / 2) + 1 = 3; the third window would start at 2 * 2 = 4 >= in + pb = 4: dropped.
    # windows: cells -1 0 -> 1; cells 1 2 -> 3
    x3 = np.arange(1, 4, dtype=np.float32).reshape(1, 1, 3)
    attrs = {"kernel_shape": [2], "strides": [2], "pads": [1, 1], "ceil_mode": 1}
    np.testing.assert_array_equal(REF["MaxPool"]([x3], attrs, 13)[0].reshape(-1), [1, 3])
    # the same windows averaged: count_include_pad 0: 1 / 1, (2 + 3) / 2; 1: (0 + 1) / 2, 2.5
    np.testing.assert_array_equal(REF["AveragePool"]([x3], attrs, 13)[0].reshape(-1), [1, 2.5])
    np.testing.assert_array_equal(REF["AveragePool"]([x3], dict(attrs, count_include_pad=1), 13)[0].reshape(-1), [0.5, 2.5])


def test_count_include_pad_pair():
    x = np.arange(1, 6, dtype=np.float32).reshape(1, 1, 5)
    # in 5, k 3, stride 2, pads [1, 1]: (7 - 3) / 2 + 1 = 3 windows over cells {-1 0 1}, {1 2 3}, {3 4 5}
    attrs = {"kernel_shape": [3], "strides": [2], "pads": [1, 1]}
    # 0: (1 + 2) / 2 = 1.5, (2 + 3 + 4) / 3 = 3, (4 + 5) / 2 = 4.5
    y, aux = REF["AveragePool"]([x], dict(attrs, count_include_pad=0), 13)
    np.testing.assert_array_equal(y.reshape(-1), [1.5, 3, 4.5])
    np.testing.assert_array_equal(aux["mag"].reshape(-1), [1.5, 3, 4.5])
    # 1: 3 / 3 = 1, 3, 9 / 3 = 3
    np.testing.assert_array_equal(REF["AveragePool"]([x], dict(attrs, count_include_pad=1), 13)[0].reshape(-1), [1, 3, 3])
    # a cell that exists only because of ceil mode is never counted: k 2, stride 2, no pads, ceil: {0 1} {2 3} {4 (5)} -> 5 / 1
    attrs = {"kernel_shape": [2], "strides": [2], "ceil_mode": 1, "count_include_pad": 1}
    np.testing.assert_array_equal(REF["AveragePool"]([x], attrs, 13)[0].reshape(-1), [1.5, 3.5, 5])


def test_softmax_before_opset_13_flattens_at_axis():
    x = np.log(np.array([[[1, 2], [3, 4], [5, 5]], [[1, 1], [2, 2], [2, 2]]], np.float64)).astype(np.float32)    # [2, 3, 2]
    # opset 11, default axis 1: rows of 3 * 2 = 6.  image 0: exp sums to 1 + 2 + 3 + 4 + 5 + 5 = 20: [0, 0, 1] = 2 / 20,
    # [0, 2, 0] = 5 / 20; image 1: sum 10: [1, 1, 0] = 2 / 10
    y = REF["Softmax"]([x], {}, 11)[0]
    np.testing.assert_allclose([y[0, 0, 1], y[0, 2, 0], y[1, 1, 0]], [0.1, 0.25, 0.2], rtol=0, atol=1e-7)
    # axis 2 at opset 11: rows of 2: [0, 0, 1] = 2 / 3; axis 0: one row of 12, sum 30: [0, 0, 1] = 2 / 30
    assert abs(REF["Softmax"]([x], {"axis": 2}, 11)[0][0, 0, 1] - 2 / 3) < 1e-7
    assert abs(REF["Softmax"]([x], {"axis": 0}, 11)[0][0, 0, 1] - 2 / 30) < 1e-7
    # opset 13: along one axis, default the last: [0, 0, 1] = 2 / 3, [0, 2, 0] = 5 / 10; axis 1: [0, 0, 1] = 2 / (2 + 4 + 5)
    y = REF["Softmax"]([x], {}, 13)[0]
    np.testing.assert_allclose([y[0, 0, 1], y[0, 2, 0]], [2 / 3, 0.5], rtol=0, atol=1e-7)
    assert abs(REF["Softmax"]([x], {"axis": 1}, 13)[0][0, 0, 1] - 2 / 11) < 1e-7


def test_pad_with_axes_modes_and_negative_pads():
    x = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    axes = np.array([-1], np.int64)

    def pad(pads, mode="constant", value=None):
        return REF["Pad"]([x, np.array(pads, np.int64), value, axes], {"mode": mode}, 18)[0]
    # pads [1, 2] on the LAST axis only: position 0 is padding, position 1 is x[:, 0]
    np.testing.assert_array_equal(pad([1, 2]), [[0, 1, 2, 3, 0, 0], [0, 4, 5, 6, 0, 0]])
    np.testing.assert_array_equal(pad([1, 0], value=np.array(7, np.float32)), [[7, 1, 2, 3], [7, 4, 5, 6]])
    # reflect [2, 1]: positions -2 -1 | 0 1 2 | 3 mirror about the ends without repeating them: 3 2 | 1 2 3 | 2
    np.testing.assert_array_equal(pad([2, 1], "reflect")[0], [3, 2, 1, 2, 3, 2])
    # edge [1, 2]: 1 | 1 2 3 | 3 3
    np.testing.assert_array_equal(pad([1, 2], "edge")[0], [1, 1, 2, 3, 3, 3])
    # a negative pad crops: [-1, 1]: position 0 is x[:, 1]: 2 3 0
    np.testing.assert_array_equal(pad([-1, 1]), [[2, 3, 0], [5, 6, 0]])
    # without axes the pads cover every axis: [b0, b1, e0, e1] = [1, 0, 0, 1] -> a row in front, a column behind
    y = REF["Pad"]([x, np.array([1, 0, 0, 1], np.int64)], {}, 13)[0]
    np.testing.assert_array_equal(y, [[0, 0, 0, 0], [1, 2, 3, 0], [4, 5, 6, 0]])


def test_small_definitions():
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    # Gather: index -1 on an axis of 3 is 2
    np.testing.assert_array_equal(REF["Gather"]([x, np.array([-1, 0], np.int64)], {"axis": 1}, 13)[0], x[:, [2, 0]])
    # Split, num_outputs 3 of an axis of 5: chunks of ceil(5 / 3) = 2, the last one smaller: 2, 2, 1
    x5 = np.arange(10, dtype=np.float32).reshape(2, 5)
    parts = REF["Split"]([x5], {"axis": 1, "num_outputs": 3}, 18)[0]
    assert [p.shape[1] for p in parts] == [2, 2, 1] and parts[2][1, 0] == 9
    # Reduce with absent / empty axes: everything, or identity with noop_with_empty_axes = 1
    assert REF["ReduceSum"]([x], {"keepdims": 0}, 13)[0] == 276
    np.testing.assert_array_equal(REF["ReduceSum"]([x, np.array([], np.int64)], {"noop_with_empty_axes": 1}, 13)[0], x)
    assert REF["ReduceSum"]([x, np.array([], np.int64)], {"keepdims": 0}, 13)[0] == 276
    # Slice: INT64 bounds clamp; a negative step walks down to (not including) the clamped end
    big = onnx_ref.INT64_MAX
    y = REF["Slice"]([x, np.array([-1], np.int64), np.array([onnx_ref.INT64_MIN], np.int64), np.array([2], np.int64), np.array([-1], np.int64)], {}, 13)[0]
    np.testing.assert_array_equal(y, x[:, :, ::-1])
    y = REF["Slice"]([x, np.array([1], np.int64), np.array([big], np.int64), np.array([2], np.int64), np.array([2], np.int64)], {}, 13)[0]
    np.testing.assert_array_equal(y, x[:, :, 1::2])
    # Flatten at axis 0 and at a negative axis
    assert REF["Flatten"]([x], {"axis": 0}, 13)[0].shape == (1, 24) and REF["Flatten"]([x], {"axis": -1}, 13)[0].shape == (6, 4)
    # Relu, Clip and MaxPool keep a NaN
    n = np.array([[[np.nan, 1.0, -2.0, 3.0]]], np.float32)
    assert np.isnan(REF["Relu"]([n], {}, 13)[0][0, 0, 0]) and np.isnan(REF["Clip"]([n, np.float32(-1), np.float32(1)], {}, 13)[0][0, 0, 0])
    y = REF["MaxPool"]([n], {"kernel_shape": [2], "strides": [2]}, 13)[0].reshape(-1)
    assert np.isnan(y[0]) and y[1] == 3
