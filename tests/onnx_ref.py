"""The ONNX operator definitions the executor's op table is held to, in numpy fp64: explicit index arithmetic, loops over output
positions, nothing from the package under test and nothing from torch.

REF[op](inputs, attrs, opset) -> (y, aux).  inputs: numpy arrays in the operator's input order (None for an absent optional input;
fp32 data is widened to fp64 here), attrs: the node's attribute dict, opset: the default-domain opset of the graph.  y: fp64 (a list
for Split; integer / bool tensors keep their type).  aux: None for an operator that only moves or selects values, else a dict with
  'mag'      per output, the sum of the magnitudes of the terms it adds up (sum |x w| (+ |b|) for a convolution, sum |x| / count for
             an average, the interpolation of |x| for a linear Resize): what a rounding-error bound of an fp32 evaluation scales with
  'min_tap'  (convolutions) per output, the smallest |x w| among the products that reach it: what the output would lose at least if a
             kernel position or a row of padding were dropped.
  'scales'   (MXQuantizeDequantize) the E8M0 scale code of every block.

QuantizeLinear / DequantizeLinear (opset 13 and 19) are defined in fp32 and compared bit for bit: they compute in fp32 and return
typed tensors (int8 / uint8 / Float8E4M3FN codes; DequantizeLinear fp32) — see that section.  MXQuantizeDequantize and BlockHadamard,
this project's own domain, defer to tests/mx_model.py and tests/mx_rotate_model.py, the definitions of record.
"""
import itertools
import math

import numpy as np

REF = {}


def ref(*names):
    def deco(fn):
        for n in names:
            REF[n] = fn
        return fn
    return deco


def _f(x):
    return np.asarray(x, np.float64)


def _ints(v):
    return [int(i) for i in np.asarray(v).reshape(-1)]


# ------------------------------------------------------------------------------------------------ padding and lengths
def auto_pads(attrs, size, k, strides, dil):
    """[b1..bn, e1..en] of a Conv / pool over spatial `size`."""
    nd = len(k)
    ap = attrs.get("auto_pad", "NOTSET")
    if ap in ("NOTSET", ""):
        return list(attrs.get("pads", [0] * (2 * nd)))
    if ap == "VALID":
        return [0] * (2 * nd)
    beg, end = [], []
    for i in range(nd):
        out = math.ceil(size[i] / strides[i])
        total = max(0, (out - 1) * strides[i] + (k[i] - 1) * dil[i] + 1 - size[i])
        b = total // 2 if ap == "SAME_UPPER" else total - total // 2
        beg.append(b)
        end.append(total - b)
    return beg + end


def pool_len(size, k, stride, dil, pb, pe, ceil):
    q = (size + pb + pe - ((k - 1) * dil + 1)) / stride
    out = (math.ceil(q) if ceil else math.floor(q)) + 1
    if ceil and (out - 1) * stride >= size + pb:       # the last window would start at or beyond the input and its begin padding
        out -= 1
    return out


# ------------------------------------------------------------------------------------------------ convolutions
@ref("Conv")
def conv(inputs, attrs, opset):
    x, w = _f(inputs[0]), _f(inputs[1])
    b = _f(inputs[2]) if len(inputs) > 2 and inputs[2] is not None else None
    nd = w.ndim - 2
    k = list(w.shape[2:])
    strides = attrs.get("strides", [1] * nd)
    dil = attrs.get("dilations", [1] * nd)
    g = int(attrs.get("group", 1))
    size = x.shape[2:]
    pads = auto_pads(attrs, size, k, strides, dil)
    out = [(size[i] + pads[i] + pads[nd + i] - ((k[i] - 1) * dil[i] + 1)) // strides[i] + 1 for i in range(nd)]
    n, cin, cout = x.shape[0], x.shape[1], w.shape[0]
    cg, og = cin // g, cout // g
    y = np.zeros((n, cout, *out))
    mag = np.zeros_like(y)
    tap = np.full_like(y, np.inf)
    for o in itertools.product(*[range(v) for v in out]):
        for t in itertools.product(*[range(v) for v in k]):
            pos = tuple(o[i] * strides[i] - pads[i] + t[i] * dil[i] for i in range(nd))
            if any(p < 0 or p >= size[i] for i, p in enumerate(pos)):
                continue                                    # a padded cell: contributes zero
            for gi in range(g):
                xs = x[(slice(None), slice(gi * cg, (gi + 1) * cg)) + pos]                 # [N, cg]
                ws = w[(slice(gi * og, (gi + 1) * og), slice(None)) + t]                   # [og, cg]
                terms = xs[:, None, :] * ws[None, :, :]                                    # [N, og, cg]
                dst = (slice(None), slice(gi * og, (gi + 1) * og)) + o
                y[dst] += terms.sum(-1)
                mag[dst] += np.abs(terms).sum(-1)
                tap[dst] = np.minimum(tap[dst], np.abs(terms).min(-1))
    if b is not None:
        shape = (1, cout) + (1,) * nd
        y += b.reshape(shape)
        mag += np.abs(b).reshape(shape)
    return y, {"mag": mag, "min_tap": tap}


def convt_pads(attrs, size, k, strides, dil, opad):
    nd = len(k)
    full = [strides[i] * (size[i] - 1) + opad[i] + (k[i] - 1) * dil[i] + 1 for i in range(nd)]
    ap = attrs.get("auto_pad", "NOTSET")
    want = attrs.get("output_shape")
    if want:
        want = list(want)[-nd:]
    elif ap in ("SAME_UPPER", "SAME_LOWER"):
        want = [size[i] * strides[i] for i in range(nd)]
    elif ap == "VALID":
        return full, [0] * (2 * nd)
    else:
        return full, list(attrs.get("pads", [0] * (2 * nd)))
    beg, end = [], []
    for i in range(nd):
        total = full[i] - want[i]
        b = total // 2 if ap == "SAME_UPPER" else total - total // 2
        beg.append(b)
        end.append(total - b)
    return full, beg + end


@ref("ConvTranspose")
def conv_transpose(inputs, attrs, opset):
    x, w = _f(inputs[0]), _f(inputs[1])                     # w: [Cin, Cout / g, k...]
    b = _f(inputs[2]) if len(inputs) > 2 and inputs[2] is not None else None
    nd = w.ndim - 2
    k = list(w.shape[2:])
    strides = attrs.get("strides", [1] * nd)
    dil = attrs.get("dilations", [1] * nd)
    opad = attrs.get("output_padding", [0] * nd)
    g = int(attrs.get("group", 1))
    size = x.shape[2:]
    full, pads = convt_pads(attrs, size, k, strides, dil, opad)
    n, cin = x.shape[0], x.shape[1]
    cg, og = cin // g, w.shape[1]
    cout = og * g
    y = np.zeros((n, cout, *full))
    mag = np.zeros_like(y)
    tap = np.full_like(y, np.inf)
    for p in itertools.product(*[range(v) for v in size]):
        for t in itertools.product(*[range(v) for v in k]):
            o = tuple(p[i] * strides[i] + t[i] * dil[i] for i in range(nd))     # where input cell p lands through kernel tap t
            for gi in range(g):
                xs = x[(slice(None), slice(gi * cg, (gi + 1) * cg)) + p]                   # [N, cg]
                ws = w[(slice(gi * cg, (gi + 1) * cg), slice(None)) + t]                   # [cg, og]
                terms = xs[:, :, None] * ws[None, :, :]                                    # [N, cg, og]
                dst = (slice(None), slice(gi * og, (gi + 1) * og)) + o
                y[dst] += terms.sum(1)
                mag[dst] += np.abs(terms).sum(1)
                tap[dst] = np.minimum(tap[dst], np.abs(terms).min(1))
    crop = (slice(None), slice(None)) + tuple(slice(pads[i], full[i] - pads[nd + i]) for i in range(nd))
    y, mag, tap = y[crop], mag[crop], tap[crop]
    if b is not None:
        shape = (1, cout) + (1,) * nd
        y = y + b.reshape(shape)
        mag = mag + np.abs(b).reshape(shape)
    return y, {"mag": mag, "min_tap": tap}


# ------------------------------------------------------------------------------------------------ pools
def _pool(inputs, attrs, avg):
    x = _f(inputs[0])
    k = list(attrs["kernel_shape"])
    nd = len(k)
    strides = attrs.get("strides", [1] * nd)
    dil = attrs.get("dilations", [1] * nd)
    ceil = bool(attrs.get("ceil_mode", 0))
    cip = bool(attrs.get("count_include_pad", 0))
    size = x.shape[2:]
    pads = auto_pads(attrs, size, k, strides, dil)
    out = [pool_len(size[i], k[i], strides[i], dil[i], pads[i], pads[nd + i], ceil) for i in range(nd)]
    y = np.zeros(x.shape[:2] + tuple(out))
    mag = np.zeros_like(y)
    for o in itertools.product(*[range(v) for v in out]):
        cells = [[o[i] * strides[i] - pads[i] + t * dil[i] for t in range(k[i])] for i in range(nd)]
        inside = [[c for c in cells[i] if 0 <= c < size[i]] for i in range(nd)]
        win = x[(slice(None), slice(None)) + np.ix_(*inside)].reshape(x.shape[0], x.shape[1], -1)
        dst = (slice(None), slice(None)) + o
        if not avg:
            y[dst] = win.max(-1)                            # (np.max: a NaN in the window is the result)
            continue
        if cip:     # cells inside the input or the explicit pads; what only ceil mode adds is never counted
            count = int(np.prod([sum(1 for c in cells[i] if -pads[i] <= c < size[i] + pads[nd + i]) for i in range(nd)]))
        else:
            count = win.shape[-1]
        y[dst] = win.sum(-1) / count
        mag[dst] = np.abs(win).sum(-1) / count
    return y, ({"mag": mag} if avg else None)


@ref("MaxPool")
def max_pool(inputs, attrs, opset):
    return _pool(inputs, attrs, False)


@ref("AveragePool")
def average_pool(inputs, attrs, opset):
    return _pool(inputs, attrs, True)


@ref("GlobalAveragePool")
def global_average_pool(inputs, attrs, opset):
    x = _f(inputs[0])
    ax = tuple(range(2, x.ndim))
    return x.mean(ax, keepdims=True), {"mag": np.abs(x).mean(ax, keepdims=True)}


@ref("GlobalMaxPool")
def global_max_pool(inputs, attrs, opset):
    x = _f(inputs[0])
    return x.max(tuple(range(2, x.ndim)), keepdims=True), None


# ------------------------------------------------------------------------------------------------ Resize / Upsample
def resize_coord(x, n_in, n_out, scale, coord):
    if coord == "half_pixel":
        return (x + 0.5) / scale - 0.5
    if coord == "pytorch_half_pixel":
        return (x + 0.5) / scale - 0.5 if n_out > 1 else 0.0
    if coord == "align_corners":
        return x * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    if coord == "asymmetric":
        return x / scale
    raise ValueError(coord)


def nearest_index(xo, n_in, nearest):
    i = {"round_prefer_floor": lambda v: math.ceil(v - 0.5), "round_prefer_ceil": lambda v: math.floor(v + 0.5),
         "floor": math.floor, "ceil": math.ceil}[nearest](xo)
    return min(max(int(i), 0), n_in - 1)


@ref("Resize", "Upsample")
def resize(inputs, attrs, opset, op_type="Resize"):
    x = _f(inputs[0])
    old = op_type == "Upsample" or opset < 11
    if old:                                                 # (X, scales): asymmetric coordinates, nearest takes the floor
        scales, sizes = inputs[1], None
        coord, nearest = "asymmetric", "floor"
    else:                                                   # (X, roi, scales, sizes)
        scales = inputs[2] if len(inputs) > 2 else None
        sizes = inputs[3] if len(inputs) > 3 else None
        coord = attrs.get("coordinate_transformation_mode", "half_pixel")
        nearest = attrs.get("nearest_mode", "round_prefer_floor")
    mode = attrs.get("mode", "nearest")
    if sizes is not None and np.asarray(sizes).size:
        out = _ints(sizes)
        scale = [out[a] / x.shape[a] for a in range(x.ndim)]
    else:
        scale = [float(v) for v in np.asarray(scales, np.float64).reshape(-1)]      # (the fp32 values, widened)
        out = [int(math.floor(x.shape[a] * scale[a])) for a in range(x.ndim)]
    mag = np.abs(x)
    for a in range(x.ndim):
        n_in = x.shape[a]
        if out[a] == n_in and scale[a] == 1.0:
            continue
        xs, ms = np.moveaxis(x, a, 0), np.moveaxis(mag, a, 0)
        y = np.zeros((out[a],) + xs.shape[1:])
        m = np.zeros_like(y)
        for o in range(out[a]):
            xo = resize_coord(o, n_in, out[a], scale[a], coord)
            if mode == "nearest":
                i = nearest_index(xo, n_in, nearest)
                y[o], m[o] = xs[i], ms[i]
            elif mode == "linear":
                xo = min(max(xo, 0.0), n_in - 1)
                i0 = int(math.floor(xo))
                i1 = min(i0 + 1, n_in - 1)
                t = xo - i0
                y[o] = (1.0 - t) * xs[i0] + t * xs[i1]
                m[o] = (1.0 - t) * ms[i0] + t * ms[i1]
            else:
                raise ValueError(mode)
        x, mag = np.moveaxis(y, 0, a), np.moveaxis(m, 0, a)
    return x, ({"mag": mag} if mode == "linear" else None)


REF["Upsample"] = lambda inputs, attrs, opset: resize(inputs, attrs, opset, "Upsample")


# ------------------------------------------------------------------------------------------------ Pad
@ref("Pad")
def pad(inputs, attrs, opset):
    x = _f(inputs[0])
    pads = _ints(inputs[1]) if len(inputs) > 1 and inputs[1] is not None else list(attrs["pads"])
    value = float(np.asarray(inputs[2]).reshape(-1)[0]) if len(inputs) > 2 and inputs[2] is not None else float(attrs.get("value", 0.0))
    axes = _ints(inputs[3]) if len(inputs) > 3 and inputs[3] is not None else list(range(x.ndim))
    axes = [a + x.ndim if a < 0 else a for a in axes]
    mode = attrs.get("mode", "constant")
    for j, a in enumerate(axes):
        b, e = pads[j], pads[len(axes) + j]
        n = x.shape[a]
        xs = np.moveaxis(x, a, 0)
        y = np.full((n + b + e,) + xs.shape[1:], value)
        for o in range(n + b + e):
            i = o - b                                       # (a negative pad: the positions start inside the input)
            if mode == "edge":
                i = min(max(i, 0), n - 1)
            elif mode == "reflect":
                i = i % (2 * (n - 1))
                i = 2 * (n - 1) - i if i >= n else i
            if 0 <= i < n:
                y[o] = xs[i]
        x = np.moveaxis(y, 0, a)
    return x, None


# ------------------------------------------------------------------------------------------------ reductions, Softmax, norms
def _reduce(fn, scaled):
    def run(inputs, attrs, opset):
        x = _f(inputs[0])
        axes = _ints(inputs[1]) if len(inputs) > 1 and inputs[1] is not None else attrs.get("axes")
        keep = bool(attrs.get("keepdims", 1))
        if axes is None or len(axes) == 0:
            if attrs.get("noop_with_empty_axes", 0):
                return x, ({"mag": np.abs(x)} if scaled else None)
            axes = list(range(x.ndim))
        axes = tuple(a + x.ndim if a < 0 else a for a in axes)
        return fn(x, axis=axes, keepdims=keep), ({"mag": fn(np.abs(x), axis=axes, keepdims=keep)} if scaled else None)
    return run


REF["ReduceSum"] = _reduce(np.sum, True)
REF["ReduceMean"] = _reduce(np.mean, True)
REF["ReduceMax"] = _reduce(np.max, False)
REF["ReduceMin"] = _reduce(np.min, False)


def _softmax_rows(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


@ref("Softmax")
def softmax(inputs, attrs, opset):
    x = _f(inputs[0])
    if opset >= 13:
        ax = int(attrs.get("axis", -1))
        return np.moveaxis(_softmax_rows(np.moveaxis(x, ax, -1)), -1, ax), None
    ax = int(attrs.get("axis", 1))
    ax = ax + x.ndim if ax < 0 else ax
    rows = int(np.prod(x.shape[:ax], dtype=np.int64))
    return _softmax_rows(x.reshape(rows, -1)).reshape(x.shape), None


@ref("BatchNormalization")
def batch_norm(inputs, attrs, opset):
    x, scale, bias, mean, var = (_f(v) for v in inputs[:5])
    sh = (1, -1) + (1,) * (x.ndim - 2)
    return (x - mean.reshape(sh)) / np.sqrt(var.reshape(sh) + float(attrs.get("epsilon", 1e-5))) * scale.reshape(sh) + bias.reshape(sh), None


@ref("LayerNormalization")
def layer_norm(inputs, attrs, opset):
    x, scale = _f(inputs[0]), _f(inputs[1])
    bias = _f(inputs[2]) if len(inputs) > 2 and inputs[2] is not None else 0.0
    ax = int(attrs.get("axis", -1))
    axes = tuple(range(ax + x.ndim if ax < 0 else ax, x.ndim))
    mean = x.mean(axes, keepdims=True)
    var = ((x - mean) ** 2).mean(axes, keepdims=True)
    return (x - mean) / np.sqrt(var + float(attrs.get("epsilon", 1e-5))) * scale + bias, None


@ref("InstanceNormalization")
def instance_norm(inputs, attrs, opset):
    x, scale, bias = (_f(v) for v in inputs[:3])
    axes = tuple(range(2, x.ndim))
    sh = (1, -1) + (1,) * (x.ndim - 2)
    mean = x.mean(axes, keepdims=True)
    var = ((x - mean) ** 2).mean(axes, keepdims=True)
    return (x - mean) / np.sqrt(var + float(attrs.get("epsilon", 1e-5))) * scale.reshape(sh) + bias.reshape(sh), None


# ------------------------------------------------------------------------------------------------ elementwise
_erf = np.vectorize(math.erf, otypes=[np.float64])


def _unary(fn):
    return lambda inputs, attrs, opset: (fn(_f(inputs[0]), attrs), None)


REF["Relu"] = _unary(lambda x, a: np.maximum(x, 0.0))
REF["LeakyRelu"] = _unary(lambda x, a: np.where(x >= 0, x, x * np.float64(np.float32(a.get("alpha", 0.01)))))
REF["Sigmoid"] = _unary(lambda x, a: 1.0 / (1.0 + np.exp(-x)))
REF["Tanh"] = _unary(lambda x, a: np.tanh(x))
REF["HardSigmoid"] = _unary(lambda x, a: np.clip(x * float(a.get("alpha", 0.2)) + float(a.get("beta", 0.5)), 0.0, 1.0))
REF["HardSwish"] = _unary(lambda x, a: x * np.clip(x / 6.0 + 0.5, 0.0, 1.0))
REF["Erf"] = _unary(lambda x, a: _erf(x))
REF["Sqrt"] = _unary(lambda x, a: np.sqrt(x))
REF["Exp"] = _unary(lambda x, a: np.exp(x))
REF["Log"] = _unary(lambda x, a: np.log(x))
REF["Abs"] = _unary(lambda x, a: np.abs(x))
REF["Neg"] = _unary(lambda x, a: -x)
REF["Reciprocal"] = _unary(lambda x, a: 1.0 / x)
REF["Floor"] = _unary(lambda x, a: np.floor(x))
REF["Ceil"] = _unary(lambda x, a: np.ceil(x))
REF["Identity"] = REF["Dropout"] = _unary(lambda x, a: x)


@ref("Gelu")
def gelu(inputs, attrs, opset):
    x = _f(inputs[0])
    if attrs.get("approximate", "none") == "tanh":
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))), None
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0))), None


@ref("PRelu")
def prelu(inputs, attrs, opset):
    x, slope = _f(inputs[0]), _f(inputs[1])
    return np.where(x >= 0, x, x * slope), None             # (slope broadcasts to x: [C, 1, 1] against [N, C, H, W])


@ref("Clip")
def clip(inputs, attrs, opset):
    x = _f(inputs[0])
    lo = inputs[1] if len(inputs) > 1 and inputs[1] is not None else attrs.get("min")
    hi = inputs[2] if len(inputs) > 2 and inputs[2] is not None else attrs.get("max")
    if lo is not None:
        x = np.maximum(x, float(np.asarray(lo).reshape(-1)[0]))
    if hi is not None:
        x = np.minimum(x, float(np.asarray(hi).reshape(-1)[0]))
    return x, None


for _n, _fn in (("Add", np.add), ("Sub", np.subtract), ("Mul", np.multiply), ("Div", np.divide), ("Pow", np.power)):
    REF[_n] = (lambda fn: (lambda inputs, attrs, opset: (fn(_f(inputs[0]), _f(inputs[1])), None)))(_fn)
REF["Eltwise"] = REF["Add"]


@ref("Where")
def where(inputs, attrs, opset):
    return np.where(np.asarray(inputs[0]).astype(bool), _f(inputs[1]), _f(inputs[2])), None


@ref("Equal")
def equal(inputs, attrs, opset):
    return np.asarray(inputs[0]) == np.asarray(inputs[1]), None


_CAST = {1: np.float32, 2: np.uint8, 3: np.int8, 6: np.int32, 7: np.int64, 9: np.bool_, 10: np.float16, 11: np.float64}


@ref("Cast")
def cast(inputs, attrs, opset):
    return np.asarray(inputs[0]).astype(_CAST[int(attrs["to"])]), None


# ------------------------------------------------------------------------------------------------ shape and index operators
@ref("Flatten")
def flatten(inputs, attrs, opset):
    x = _f(inputs[0])
    ax = int(attrs.get("axis", 1))
    ax = ax + x.ndim if ax < 0 else ax
    return x.reshape(int(np.prod(x.shape[:ax], dtype=np.int64)), -1), None


@ref("Reshape")
def reshape(inputs, attrs, opset):
    x = _f(inputs[0])
    shp = _ints(inputs[1])
    if not attrs.get("allowzero", 0):
        shp = [x.shape[i] if d == 0 else d for i, d in enumerate(shp)]
    return x.reshape(shp), None


@ref("Transpose")
def transpose(inputs, attrs, opset):
    x = _f(inputs[0])
    return np.transpose(x, attrs.get("perm") or list(reversed(range(x.ndim)))), None


@ref("Concat")
def concat(inputs, attrs, opset):
    return np.concatenate([_f(v) for v in inputs], int(attrs["axis"])), None


@ref("Split")
def split(inputs, attrs, opset):
    x = _f(inputs[0])
    ax = int(attrs.get("axis", 0))
    sizes = _ints(inputs[1]) if len(inputs) > 1 and inputs[1] is not None else attrs.get("split")
    if sizes is None:
        n = int(attrs["num_outputs"])
        chunk = math.ceil(x.shape[ax] / n)                  # chunks of ceil(dim / n), the last one smaller
        sizes = [chunk] * (n - 1) + [x.shape[ax] - chunk * (n - 1)]
    out, start = [], 0
    for k in sizes:
        out.append(np.take(x, range(start, start + k), ax))
        start += k
    return out, None


INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63


@ref("Slice")
def slice_(inputs, attrs, opset):
    x = _f(inputs[0])
    starts = _ints(inputs[1]) if len(inputs) > 1 and inputs[1] is not None else attrs["starts"]
    ends = _ints(inputs[2]) if len(inputs) > 2 and inputs[2] is not None else attrs["ends"]
    axes = _ints(inputs[3]) if len(inputs) > 3 and inputs[3] is not None else attrs.get("axes", list(range(len(starts))))
    steps = _ints(inputs[4]) if len(inputs) > 4 and inputs[4] is not None else [1] * len(starts)
    for st, en, ax, sp in zip(starts, ends, axes, steps):
        n = x.shape[ax]
        st = st + n if st < 0 else st
        en = en + n if en < 0 else en
        if sp > 0:
            st, en = min(max(st, 0), n), min(max(en, 0), n)
        else:
            st, en = min(max(st, 0), n - 1), min(max(en, -1), n - 1)
        idx, i = [], st
        while (i < en) if sp > 0 else (i > en):
            idx.append(i)
            i += sp
        x = np.take(x, idx, ax)
    return x, None


@ref("Gather")
def gather(inputs, attrs, opset):
    x, idx = _f(inputs[0]), np.asarray(inputs[1]).astype(np.int64)
    ax = int(attrs.get("axis", 0))
    idx = np.where(idx < 0, idx + x.shape[ax], idx)         # index i < 0 means i + dim
    return np.take(x, idx, ax), None


@ref("Squeeze")
def squeeze(inputs, attrs, opset):
    x = _f(inputs[0])
    axes = _ints(inputs[1]) if len(inputs) > 1 and inputs[1] is not None else attrs.get("axes")
    return (np.squeeze(x) if axes is None else np.squeeze(x, tuple(axes))), None


@ref("Unsqueeze")
def unsqueeze(inputs, attrs, opset):
    x = _f(inputs[0])
    axes = _ints(inputs[1]) if len(inputs) > 1 and inputs[1] is not None else attrs.get("axes")
    return np.expand_dims(x, tuple(axes)), None


@ref("Expand")
def expand(inputs, attrs, opset):
    x = _f(inputs[0])
    return np.broadcast_to(x, np.broadcast_shapes(x.shape, tuple(_ints(inputs[1])))), None


@ref("Shape")
def shape(inputs, attrs, opset):
    return np.asarray(np.asarray(inputs[0]).shape, np.int64), None


@ref("ConstantOfShape")
def constant_of_shape(inputs, attrs, opset):
    v = attrs.get("value")
    v = np.asarray(v).reshape(-1)[0] if v is not None else np.float32(0.0)
    return np.full(_ints(inputs[0]), v), None


# ------------------------------------------------------------------------------------------------ matrix products
@ref("MatMul")
def matmul(inputs, attrs, opset):
    a, b = _f(inputs[0]), _f(inputs[1])
    return np.matmul(a, b), {"mag": np.matmul(np.abs(a), np.abs(b))}


@ref("Gemm")
def gemm(inputs, attrs, opset):
    """Y = alpha A' B' + beta C: A' = A^T if transA, B' = B^T if transB, C broadcast to [M, N]."""
    a, b = _f(inputs[0]), _f(inputs[1])
    c = _f(inputs[2]) if len(inputs) > 2 and inputs[2] is not None else None
    a = a.T if attrs.get("transA", 0) else a
    b = b.T if attrs.get("transB", 0) else b
    alpha, beta = float(attrs.get("alpha", 1.0)), float(attrs.get("beta", 1.0))
    y, mag = alpha * (a @ b), abs(alpha) * (np.abs(a) @ np.abs(b))
    if c is not None:
        y, mag = y + beta * c, mag + np.abs(beta * c)
    return y, {"mag": mag}


# ------------------------------------------------------------------------------------------------ QuantizeLinear / DequantizeLinear
# Written from the operator text (opset 13 and 19).  These two are defined in the operator's own float type, fp32, and their tests
# are bit for bit: x and the scales are taken as fp32, x / y_scale is ONE fp32 division, (x - zero_point) * x_scale one fp32
# product, and DequantizeLinear returns fp32 (not the fp64 of the other entries).  A quantised tensor keeps its type: np.int8,
# np.uint8, or Float8E4M3FN — one e4m3fn code per element.
class Float8E4M3FN(np.ndarray):
    """A tensor of ONNX type FLOAT8E4M3FN (17) as its codes: a uint8 array that remembers what it is.  1 sign bit, 4 exponent bits
    (bias 7), 3 mantissa bits; exponent 0 is subnormal (m 2^-9); no infinities; 0x7f / 0xff are NaN; largest finite 0x7e = 448."""

    def __new__(cls, codes):
        return np.require(codes, np.uint8, "C").view(cls)


def _e4m3fn_values():
    """The values of the codes 0x00 .. 0x7e, ascending, from the encoding."""
    code = np.arange(127)
    e, m = code >> 3, code & 7
    return np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))


E4M3FN_VALUES = _e4m3fn_values()


def e4m3fn_decode(codes):
    c = np.asarray(codes).view(np.uint8)
    mag = np.where((c & 0x7F) == 0x7F, np.nan, E4M3FN_VALUES[np.minimum(c & 0x7F, 126)])
    return np.where(c & 0x80, -mag, mag).astype(np.float32)


def e4m3fn_encode(v, saturate=True):
    """Cast fp32 -> float8e4m3fn as the Cast / QuantizeLinear text tabulates it: to the nearest value, a tie to the code with the
    even mantissa; NaN stays NaN; the sign of zero is kept; out of range (beyond the tie with the 480 the format does not have,
    and +-inf): +-448 with saturate = 1, NaN without."""
    v = np.asarray(v, np.float32)
    a = np.abs(v.astype(np.float64))
    nan = np.isnan(a)
    over = a > 464.0
    a = np.where(nan, 0.0, np.minimum(a, 448.0))
    hi = np.minimum(np.searchsorted(E4M3FN_VALUES, a, "left"), 126)            # the first code whose value is >= a
    lo = np.maximum(hi - 1, 0)
    d_lo, d_hi = a - E4M3FN_VALUES[lo], E4M3FN_VALUES[hi] - a
    code = np.where(d_hi < d_lo, hi, np.where(d_lo < d_hi, lo, np.where(hi % 2 == 0, hi, lo)))      # (the code's lowest bit is the mantissa's)
    code = np.where(nan | (over & (not saturate)), 0x7F, code)
    return Float8E4M3FN((code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8))


def _per_axis(p, x, axis, what):
    """A scale / zero point against x: a scalar (or one element) for the whole tensor, or 1-D along `axis`, one per slice."""
    p = np.asarray(p)
    if p.size == 1:
        return p.reshape(())
    axis = axis + x.ndim if axis < 0 else axis
    if p.ndim != 1 or not 0 <= axis < x.ndim or p.shape[0] != x.shape[axis]:
        raise ValueError(f"{what}: shape {p.shape} against axis {axis} of a tensor of shape {x.shape}")
    return p.reshape([-1 if d == axis else 1 for d in range(x.ndim)])


@ref("QuantizeLinear")
def quantize_linear(inputs, attrs, opset):
    """y = saturate(round_half_even(x / y_scale) + y_zero_point), in the type of y_zero_point (absent: uint8 zero): [-128, 127]
    for int8, [0, 255] for uint8.  float8e4m3fn (opset 19): y = cast(x / y_scale), attribute saturate (default 1); the zero point
    only names the type.  The text gives a NaN no integer code: here it takes the lower end, as a conversion that saturates does."""
    x = np.asarray(inputs[0], np.float32)
    zp = inputs[2] if len(inputs) > 2 and inputs[2] is not None else np.zeros((), np.uint8)
    axis = int(attrs.get("axis", 1))
    scale = _per_axis(np.asarray(inputs[1], np.float32), x, axis, "y_scale")
    with np.errstate(all="ignore"):
        r = (x / scale).astype(np.float32)                  # the operator's float type: one fp32 division
    if isinstance(zp, Float8E4M3FN):
        if opset < 19:
            raise ValueError(f"QuantizeLinear: a float8e4m3fn zero point at opset {opset} (19 or later)")
        return e4m3fn_encode(r, bool(attrs.get("saturate", 1))), None
    zp = np.asarray(zp)
    if zp.dtype not in (np.int8, np.uint8):
        raise ValueError(f"QuantizeLinear: zero point of type {zp.dtype}")
    info = np.iinfo(zp.dtype)
    with np.errstate(all="ignore"):
        q = np.rint(r.astype(np.float64)) + _per_axis(zp, x, axis, "y_zero_point").astype(np.float64)
    q = np.where(np.isnan(q), info.min, np.clip(q, info.min, info.max))
    return q.astype(zp.dtype), None


@ref("DequantizeLinear")
def dequantize_linear(inputs, attrs, opset):
    """y = (x - x_zero_point) * x_scale: the difference is exact (integers; a float8e4m3fn against its zero), the product fp32."""
    x = inputs[0]
    zp = inputs[2] if len(inputs) > 2 and inputs[2] is not None else None
    if zp is not None and (type(zp) is not type(x) if isinstance(x, Float8E4M3FN) or isinstance(zp, Float8E4M3FN)
                           else np.asarray(zp).dtype != np.asarray(x).dtype):
        raise ValueError("DequantizeLinear: x and x_zero_point differ in type")
    axis = int(attrs.get("axis", 1))
    f8 = isinstance(x, Float8E4M3FN)
    xv = e4m3fn_decode(x) if f8 else np.asarray(x).astype(np.int32)
    scale = _per_axis(np.asarray(inputs[1], np.float32), xv, axis, "x_scale")
    if zp is not None:
        zv = _per_axis(e4m3fn_decode(zp) if f8 else np.asarray(zp).astype(np.int32), xv, axis, "x_zero_point")
        xv = xv - zv
    with np.errstate(all="ignore"):
        return (xv.astype(np.float32) * scale).astype(np.float32), None


def qdq_pair(x, scale, zp, attrs, opset):
    """DequantizeLinear(QuantizeLinear(x)) with the same scale, zero point and attributes -> (y fp32, the codes)."""
    q, _ = quantize_linear([x, scale, zp], attrs, opset)
    y, _ = dequantize_linear([q, scale, zp], attrs, opset)
    return y, q


# ------------------------------------------------------------------------------------------------ this project's domain
_MX_ELEM = {"float8e4m3fn": "mxfp8", "float4e2m1": "mxfp4"}


@ref("MXQuantizeDequantize")
def mx_quantize_dequantize(inputs, attrs, opset):
    """The block-scaled Q/DQ of --mx: tests/mx_model.py is the definition.  aux: the E8M0 scale codes, [outer, blocks, inner]."""
    import mx_model
    if int(attrs.get("block_size", mx_model.BLOCK)) != mx_model.BLOCK:
        raise ValueError(f"MXQuantizeDequantize: block_size {attrs.get('block_size')}")
    y, scales = mx_model.fake_quant_mx(np.asarray(inputs[0], np.float32), int(attrs["axis"]), _MX_ELEM[attrs["elem_type"]], return_scales=True)
    return y, {"scales": scales}


@ref("BlockHadamard")
def block_hadamard(inputs, attrs, opset):
    """x . blockdiag(H32) along the last axis, fp32, stage by stage: tests/mx_rotate_model.py is the definition."""
    import mx_rotate_model
    if int(attrs.get("block_size", mx_rotate_model.BLOCK)) != mx_rotate_model.BLOCK:
        raise ValueError(f"BlockHadamard: block_size {attrs.get('block_size')}")
    return mx_rotate_model.fwht32(np.asarray(inputs[0], np.float32)), None
