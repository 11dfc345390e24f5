"""One table of sample calls for every `torch.ops.dipoorlet.*` op (dipoorlet_amd/torch_ops.py): CASES[op] is a list of Case(id,
build, layout), build(device) -> (args, kwargs) with new tensors on every call.  Plain data and small builders — nothing here
touches a GPU at import, and under a FakeTensorMode the builders return fake tensors of the same shapes, dtypes and strides (the
values are then never written).  The inputs are the smallest that still exercise an op's shape arithmetic: MX block axes of
K = 40 (pads to 64) and K = 32, a block axis that is not the last, per-tensor and per-channel parameters, a batched and an unbatched
B for mx_gemm, two tensors of different rank for the list ops.  Every op with a float tensor input it may be handed in any layout
also has cases whose input is dense but NOT contiguous (layout != "contig"): a transposed 2-D view ("t2d"), a channels-last 4-D
tensor ("cl4d"), transpose(0, 2) of a 3-D one ("t02").  (gptq_block / gptq_mx_block take contiguous matrices by contract — w is
written in place — and have none.)

registered_ops() is the set of ops the library itself holds in the `dipoorlet` namespace: a test holds CASES to it, so an op added
without cases fails."""
import collections
import zlib

import numpy as np
import torch

import mx_gemm_model as G

Case = collections.namedtuple("Case", "id build layout")

# layout -> the order of the axes in memory, outermost first (None: as given)
LAYOUTS = {"contig": None, "t2d": (1, 0), "cl4d": (0, 2, 3, 1), "t02": (2, 1, 0)}
NONCONTIG = ("t2d", "cl4d", "t02")


def registered_ops():
    import dipoorlet_amd.torch_ops  # noqa: F401
    return sorted(n.split("::")[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("dipoorlet::"))


def place(a, device, layout="contig"):
    """The array `a` as a tensor of a's shape on `device` whose memory order is `layout`'s; under a FakeTensorMode: a fake one."""
    a = np.asarray(a)
    perm = LAYOUTS[layout]
    if perm is None:
        c = torch.from_numpy(np.ascontiguousarray(a))
    else:
        assert a.ndim == len(perm), (layout, a.shape)
        inv = [perm.index(i) for i in range(a.ndim)]
        c = torch.from_numpy(np.ascontiguousarray(a.transpose(perm))).permute(inv)
        assert tuple(c.shape) == a.shape and not c.is_contiguous(), (layout, a.shape)
    out = torch.empty_strided(c.shape, c.stride(), dtype=c.dtype, device=device)
    if not isinstance(out, torch._subclasses.FakeTensor):
        out.copy_(c)
    return out


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))     # (the same data in every process: hash() of a str is salted)


def _normal(shape, *key, spread=3.0):
    return (_rng("x", shape, *key).standard_normal(shape) * spread).astype(np.float32)


# the logical shape each layout is shown at, for ops that take a tensor of any rank
ANY_RANK = {"contig": (3, 5, 7), "t2d": (6, 4), "cl4d": (2, 8, 5, 5), "t02": (3, 4, 5)}


def _per_layout(shapes, make, layouts=("contig",) + NONCONTIG, tag=""):
    return [Case(f"{tag}{lay}-{'x'.join(map(str, shapes[lay]))}", make(shapes[lay], lay), lay) for lay in layouts if lay in shapes]


# ------------------------------------------------------------------------------------------------ statistics
def _minmax():
    return _per_layout(ANY_RANK, lambda s, lay: lambda dev: ((place(_normal(s, "minmax"), dev, lay),), {}))


def _octav():
    out = []
    for dyn in (False, True):
        out += _per_layout(ANY_RANK, lambda s, lay: lambda dev: ((place(_normal(s, "octav"), dev, lay), dyn), {}), tag=f"dyn{int(dyn)}-")
    return out


def _abs_hist_():
    def make(s, lay):
        return lambda dev: ((place(_normal(s, "abs_hist"), dev, lay), 3.0, 16, place(np.zeros(16, np.int64), dev)), {})
    return _per_layout(ANY_RANK, make)


# the list ops: two tensors of different rank (and, for octav_batched, one batch size in front)
LISTS = {"contig": (((6, 4), "contig"), ((2, 8, 5, 5), "contig")),
         "t2d+cl4d": (((6, 4), "t2d"), ((2, 8, 5, 5), "cl4d")),
         "t02+contig": (((3, 4, 5), "t02"), ((6, 4), "contig"))}
BATCHED = {"contig": (((2, 12), "contig"), ((2, 8, 5, 5), "contig")),
           "t2d+cl4d": (((2, 12), "t2d"), ((2, 8, 5, 5), "cl4d")),
           "t02+contig": (((2, 4, 5), "t02"), ((2, 12), "contig"))}


def _xs(spec, dev, key):
    return [place(_normal(s, key, t), dev, lay) for t, (s, lay) in enumerate(spec)]


def _list_cases(table, make):
    return [Case(name, make(spec), name) for name, spec in table.items()]      # (layout: the table's key, "contig" or what is not)


def _minmax_batched():
    def make(spec):
        def build(dev):
            T = len(spec)
            return (_xs(spec, dev, "mmb"), place(np.full(T, np.inf, np.float32), dev), place(np.full(T, -np.inf, np.float32), dev)), {}
        return build
    return _list_cases(LISTS, make)


def _abs_hist_batched_():
    def make(spec):
        def build(dev):
            T = len(spec)
            return (_xs(spec, dev, "ahb"), place(np.full(T, -2.5, np.float32), dev), place(np.array([3.0, 4.0], np.float32), dev), 16,
                    place(np.zeros((T, 16), np.int64), dev)), {}
        return build
    return _list_cases(LISTS, make)


def _octav_batched():
    return _list_cases(BATCHED, lambda spec: lambda dev: ((_xs(spec, dev, "ob"), False), {}))


def hist_of(bins, seed):
    """A |normal| histogram over (0, max): the shape of what the calibration passes hand the searches."""
    x = np.abs(np.random.default_rng(seed).standard_normal(20000)).astype(np.float32)
    h = np.histogram(x, bins, (0.0, float(x.max())))[0].astype(np.int64)
    return h, np.float32(-x.max() / 2), np.float32(x.max())


def _hist_percentile():
    def make(bins, thr):
        def build(dev):
            h, lo, hi = hist_of(bins, bins)
            return (place(h, dev), float(lo), float(hi), thr), {}
        return build
    return [Case(f"bins{b}-thr{t}", make(b, t), "contig") for b, t in ((64, 0.999), (100, 0.99999))]


def _hist_kl():
    def make(bins, levels):
        def build(dev):
            h, lo, hi = hist_of(bins, bins + levels)
            return (place(h, dev), float(lo), float(hi), levels), {}
        return build
    return [Case(f"bins{b}-L{L}", make(b, L), "contig") for b, L in ((256, 32), (100, 16))]


def _hist_qmse():
    def make(bins, qtype, bw, first):
        def build(dev):
            h, lo, hi = hist_of(bins, bins + first)
            return (place(h, dev), float(lo), float(hi), qtype, bw, first), {}
        return build
    return [Case(f"bins{b}-{q}{bw}-first{f}", make(b, q, bw, f), "contig")
            for b, q, bw, f in ((256, "Linear", 8, 32), (100, "Linear", 4, 8), (256, "Float8E4M3FN", 8, 32))]


def _rowwise_minmax():
    return _per_layout({"contig": (5, 7), "t2d": (6, 4)}, lambda s, lay: lambda dev: ((place(_normal(s, "rw"), dev, lay),), {}))


def _colwise_absmax():
    return _per_layout(ANY_RANK, lambda s, lay: lambda dev: ((place(_normal(s, "cw"), dev, lay),), {}))


# ------------------------------------------------------------------------------------------------ the Q/DQ pair
def fq_params(shape, axis, signed, *key):
    """(scale fp32, zero point int32, qlo, qhi): per tensor (axis None) or one per channel of `axis`, a third of the scales powers
    of two; zero points != 0 on the unsigned grid, their int8 storage forms on the signed one."""
    n = 1 if axis is None else shape[axis]
    rng = _rng("fq", shape, axis, signed, *key)
    scale = rng.uniform(0.01, 0.1, n).astype(np.float32)
    scale[::3] = np.float32(2.0) ** rng.integers(-6, -2, scale[::3].size)
    zp = rng.integers(1, 255, n).astype(np.int32)
    if signed:
        zp = np.where(zp > 127, zp - 256, zp).astype(np.int32)
    return scale, zp, (-128 if signed else 0), (127 if signed else 255)


# (axis, signed grid?) per layout: per tensor (None) and per channel, the last axis once as -1 and the first as -dim
FQ_AXES = {"contig": ((None, True), (1, False), (-1, False)), "t2d": ((None, True), (1, False), (0, False)),
           "cl4d": ((None, False), (1, False)), "t02": ((2, True), (-3, False))}


def _fake_quant(pre):
    out = []
    for lay, shape in ANY_RANK.items():
        for axis, signed in FQ_AXES[lay]:
            def build(dev, lay=lay, shape=shape, axis=axis, signed=signed):
                scale, zp, qlo, qhi = fq_params(shape, axis, signed, pre)
                x = place(_normal(shape, "fq", pre), dev, lay)
                second = (place(_normal(shape, "fq2", pre), dev, lay),) if pre == "add_relu" else ()
                return (x,) + second + (place(scale, dev), place(zp, dev), 0 if axis is None else axis, qlo, qhi), {}
            out.append(Case(f"{lay}-{'x'.join(map(str, shape))}-axis{axis}-{'i8' if signed else 'u8'}", build, lay))
    return out


def _fake_quant_fp8():
    out = []
    for lay, shape in ANY_RANK.items():
        for axis, _ in FQ_AXES[lay]:
            def build(dev, lay=lay, shape=shape, axis=axis):
                scale = fq_params(shape, axis, True, "fp8")[0]
                return (place(_normal(shape, "fp8", spread=30.0), dev, lay), place(scale, dev), 0 if axis is None else axis), {}
            out.append(Case(f"{lay}-{'x'.join(map(str, shape))}-axis{axis}", build, lay))
    return out


def _fake_quant_set():
    def make(spec):
        def build(dev):
            xs = _xs(spec, dev, "fqs")
            shape1 = spec[1][0]
            per_ch = len(shape1) > 2          # the 4-D member: per channel on axis 1; every other member per tensor
            s0, z0, lo0, hi0 = fq_params(spec[0][0], None, True, "set0")
            s1, z1, lo1, hi1 = fq_params(shape1, 1 if per_ch else None, False, "set1")
            inner = int(np.prod(shape1[2:])) if per_ch else 1
            return (xs, [place(s0, dev), place(s1, dev)], [place(z0, dev), place(z1, dev)], [1, inner], [lo0, lo1], [hi0, hi1]), {}
        return build
    return _list_cases(LISTS, make)


# ------------------------------------------------------------------------------------------------ Microscaling
# (shape, block axis) per layout: K = 40 (pads to 64) and K = 32, along the last axis and along one that is not
MX_SHAPES = (("contig", (3, 40), -1), ("contig", (3, 32), 1), ("contig", (2, 40, 3), 1), ("contig", (2, 32, 3), -2),
             ("t2d", (4, 40), -1), ("t2d", (40, 4), 0), ("cl4d", (2, 40, 2, 2), 1), ("cl4d", (2, 3, 2, 32), 3), ("t02", (3, 32, 2), 1),
             ("t02", (2, 3, 40), -1))
ELEMS = ("mxfp8", "mxfp4")


def _mx_cases(make):
    """Both element formats at the contiguous shapes, the two in turn at the others."""
    return [Case(f"{lay}-{'x'.join(map(str, shape))}-axis{axis}-{elem}", make(lay, shape, axis, elem), lay)
            for i, (lay, shape, axis) in enumerate(MX_SHAPES) for elem in (ELEMS if lay == "contig" else (ELEMS[i % 2],))]


def _fake_quant_mx():
    return _mx_cases(lambda lay, shape, axis, elem: lambda dev: ((place(_normal(shape, "mx"), dev, lay), axis, elem), {}))


def _mx_encode():
    return _mx_cases(lambda lay, shape, axis, elem: lambda dev: ((place(_normal(shape, "enc"), dev, lay), axis, elem), {}))


def _mx_scale_search():
    return _mx_cases(lambda lay, shape, axis, elem: lambda dev: ((place(_normal(shape, "ss"), dev, lay), axis, elem), {}))


def block_shape(shape, axis):
    axis %= len(shape)
    return tuple(shape[:axis]) + (-(-shape[axis] // 32),) + tuple(shape[axis + 1:])


def packed_shapes(shape, axis, elem):
    """What the docstring of ops.mx_encode states: K-innermost, the block axis padded to a multiple of 32."""
    axis %= len(shape)
    kp = 32 * -(-shape[axis] // 32)
    lead = tuple(shape[:axis]) + tuple(shape[axis + 1:])
    return lead + (kp // 2 if elem == "mxfp4" else kp,), lead + (kp // 32,)


def _fake_quant_mx_scaled():
    def make(lay, shape, axis, elem):
        def build(dev):
            scales = _rng("sc", shape, axis, elem).integers(122, 132, block_shape(shape, axis)).astype(np.uint8)
            return (place(_normal(shape, "mxs"), dev, lay), axis, elem, place(scales, dev)), {}
        return build
    return _mx_cases(make)


def _mx_decode():
    def make(lay, shape, axis, elem):
        def build(dev):
            cs, ss = packed_shapes(shape, axis, elem)
            rng = _rng("dec", shape, axis, elem)
            return (place(rng.integers(0, 256, cs).astype(np.uint8), dev), place(rng.integers(118, 136, ss).astype(np.uint8), dev), elem,
                    list(shape), axis), {}
        return build
    return [c for c in _mx_cases(make) if c.layout == "contig"]


EXACT_VALUES = np.array([0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6], np.float64)     # every partial sum of a few of these is exact in fp32


def exact_operand(rng, lead, rows, k, elem):
    """Codes and scales of [*lead, rows, Kp] data whose products sum exactly; the elements past k are pad: code 0."""
    kp = 32 * -(-k // 32)
    v = rng.choice(EXACT_VALUES, size=tuple(lead) + (rows, kp))
    v[..., k:] = 0.0
    return G.codes_from_values(v, elem), rng.integers(125, 130, size=tuple(lead) + (rows, kp // 32)).astype(np.uint8)


def _mx_gemm():
    def make(lead, b_lead, m, n, k, ea, eb):
        def build(dev):
            rng = _rng("gemm", lead, b_lead, m, n, k, ea, eb)
            ac, a_s = exact_operand(rng, lead, m, k, ea)
            bc, b_s = exact_operand(rng, b_lead, n, k, eb)
            return (place(ac, dev), place(a_s, dev), place(bc, dev), place(b_s, dev), ea, eb), {}
        return build
    rows = (((), (), 5, 3, 40, "mxfp8", "mxfp8"), ((2,), (), 5, 3, 32, "mxfp4", "mxfp8"), ((2,), (2,), 17, 9, 40, "mxfp8", "mxfp4"),
            ((2, 3), (2, 3), 3, 2, 32, "mxfp4", "mxfp4"))
    return [Case(f"A{list(r[0])}-B{list(r[1])}-m{r[2]}n{r[3]}k{r[4]}-{r[5]}-{r[6]}", make(*r), "contig") for r in rows]


def _hadamard32():
    shapes = {"contig": (3, 64), "t2d": (5, 32), "cl4d": (2, 3, 2, 32), "t02": (3, 2, 32)}
    out = _per_layout(shapes, lambda s, lay: lambda dev: ((place(_normal(s, "had"), dev, lay),), {}))
    return out + [Case("contig-2x3x32", lambda dev: ((place(_normal((2, 3, 32), "had3"), dev),), {}), "contig")]


# ------------------------------------------------------------------------------------------------ GPTQ
def gptq_factor(k, seed):
    """An upper-triangular fp32 [k, k] with a positive diagonal: the shape of the Cholesky factor GPTQ's recursion reads."""
    rng = np.random.default_rng(seed)
    u = np.triu(rng.standard_normal((k, k)) * 0.1)
    u[np.arange(k), np.arange(k)] = rng.uniform(0.5, 1.5, k)
    return u.astype(np.float32)


def _gptq_block():
    def make(rows, k, c0, nb, per_row, fmt):
        def build(dev):
            scale, zp, qlo, qhi = fq_params((rows, k), 0 if per_row else None, False, "gptq", fmt)
            return (place(_normal((rows, k), "gw", spread=1.0), dev), c0, nb, place(gptq_factor(k, k + c0), dev), place(scale, dev),
                    place(zp, dev), qlo, qhi, fmt), {}
        return build
    rows = ((5, 40, 8, 16, True, "int"), (5, 40, 0, 40, False, "int"), (3, 32, 16, 16, True, "e4m3"), (5, 40, 32, 8, False, "e4m3"))
    return [Case(f"{r[0]}x{r[1]}-c{r[2]}+{r[3]}-{'row' if r[4] else 'tensor'}-{r[5]}", make(*r), "contig") for r in rows]


def _gptq_mx_block():
    def make(rows, k, c0, nb, elem):
        return lambda dev: ((place(_normal((rows, k), "gmw", spread=1.0), dev), c0, nb, place(gptq_factor(k, k + c0 + 1), dev), elem), {})
    rows = ((5, 40, 0, 32, "mxfp8"), (5, 40, 32, 8, "mxfp4"), (3, 32, 0, 32, "mxfp4"), (3, 64, 0, 64, "mxfp8"), (5, 40, 0, 40, "mxfp8"))
    return [Case(f"{r[0]}x{r[1]}-c{r[2]}+{r[3]}-{r[4]}", make(*r), "contig") for r in rows]


CASES = {
    "minmax": _minmax(),
    "minmax_batched": _minmax_batched(),
    "abs_hist_": _abs_hist_(),
    "abs_hist_batched_": _abs_hist_batched_(),
    "hist_percentile": _hist_percentile(),
    "hist_kl": _hist_kl(),
    "hist_qmse": _hist_qmse(),
    "octav": _octav(),
    "octav_batched": _octav_batched(),
    "rowwise_minmax": _rowwise_minmax(),
    "colwise_absmax": _colwise_absmax(),
    "fake_quant": _fake_quant(None),
    "fake_quant_relu": _fake_quant("relu"),
    "fake_quant_add_relu": _fake_quant("add_relu"),
    "fake_quant_fp8": _fake_quant_fp8(),
    "fake_quant_set": _fake_quant_set(),
    "fake_quant_mx": _fake_quant_mx(),
    "mx_encode": _mx_encode(),
    "mx_decode": _mx_decode(),
    "mx_gemm": _mx_gemm(),
    "mx_scale_search": _mx_scale_search(),
    "fake_quant_mx_scaled": _fake_quant_mx_scaled(),
    "hadamard32": _hadamard32(),
    "gptq_block": _gptq_block(),
    "gptq_mx_block": _gptq_mx_block(),
}

# ops whose float tensor inputs may come in any layout: each has at least one case of every layout its rank allows
TAKES_ANY_LAYOUT = ("minmax", "minmax_batched", "abs_hist_", "abs_hist_batched_", "octav", "octav_batched", "rowwise_minmax",
                    "colwise_absmax", "fake_quant", "fake_quant_relu", "fake_quant_add_relu", "fake_quant_fp8", "fake_quant_set",
                    "fake_quant_mx", "mx_encode", "mx_scale_search", "fake_quant_mx_scaled", "hadamard32")


def all_cases():
    return [(op, c) for op, cs in CASES.items() for c in cs]


def case_ids():
    return [f"{op}-{c.id}" for op, c in all_cases()]
