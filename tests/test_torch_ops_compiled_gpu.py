"""GPU: the Python boundary of `torch.ops.dipoorlet.*` (dipoorlet_amd/torch_ops.py) held to what it promises a compiler, over the
table of sample calls (tests/torch_op_cases.py):

1. per case, the real op against its fake kernel — count, shape, dtype, device and stride() of every output —; a case whose input
   is dense but not contiguous gives the bits the op gives on x.contiguous(); and that contiguous result is the project's
   definition of the op (DEFS: the numpy models the kernel tests use), with no tolerance: bit patterns, NaN in the same places
   (mx_gemm, on exactly representable data: equal values, a zero's sign free, as tests/test_mx_gemm_gpu.py compares them).
   octav / octav_batched / minmax_batched / abs_hist_batched_ have no entry in DEFS: tests/test_torch_ops.py holds them to the
   oracle; here they are held to their fake kernels and to their contiguous selves.
2. torch.library.opcheck on one contiguous and one non-contiguous case per op: test_schema, test_faketensor,
   test_autograd_registration (the ops have no autograd: it confirms that) and test_aot_dispatch_dynamic, the last one left out
   only for the ops of AOT_DYNAMIC_EXCEPTIONS, each with the checker's limit that is the reason.
3. four small functions through torch.compile(backend="aot_eager", fullgraph=True) — a graph break is an error — against the same
   function run eagerly, bit for bit, mutated arguments included.  (The inductor backend is not run here.)"""
import gc
import time

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import dipoorlet_amd.torch_ops  # noqa: F401
import fp8_model
import gptq_model
import kl_model
import mx_gemm_model as G
import mx_gptq_model
import mx_model
import mx_pack_model as P
import mx_rotate_model
import mx_scale_model as S
import qmse_model
import torch_op_cases as T
from oracle import np_oracle as O
from test_torch_ops_fake import outputs_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    yield
    gc.collect()


def _op(name):
    return getattr(torch.ops.dipoorlet, name)


def _tensors(args):
    """(position, tensor) of every tensor among the arguments; a tensor of a list argument has position (i, j)."""
    out = []
    for i, a in enumerate(args):
        if isinstance(a, torch.Tensor):
            out.append((i, a))
        elif isinstance(a, (list, tuple)):
            out += [((i, j), t) for j, t in enumerate(a) if isinstance(t, torch.Tensor)]
    return out


def _map(args, fn):
    return tuple(fn(a) if isinstance(a, torch.Tensor) else [fn(t) if isinstance(t, torch.Tensor) else t for t in a] if isinstance(a, list)
                 else a for a in args)


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(got, want, what):
    got, want = _host(got) if isinstance(got, torch.Tensor) else got, _host(want) if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, (what, bad.size, bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


def _same_as_definition(got, want, what, values_only=False):
    """Bit patterns equal and NaN in the same places (a NaN's payload is not part of a definition); values_only: equal as values."""
    got, want = _host(got), np.ascontiguousarray(want)
    assert got.shape == tuple(want.shape) and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    else:
        g, w = got.reshape(-1), want.reshape(-1)
        gn, wn = np.isnan(g), np.isnan(w)
        bad = np.flatnonzero((gn != wn) | (~wn & ((g != w) if values_only else (_bits(g) != _bits(w)))))
    assert bad.size == 0, (what, bad.size, bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


# ------------------------------------------------------------------------------------------------ the definitions
def _fq(pre):
    def want(a):
        if pre == "add_relu":
            x, x2, sc, zp, axis, qlo, qhi = a
            with np.errstate(invalid="ignore"):
                x = np.maximum((x + x2).astype(np.float32), np.float32(0))
        else:
            x, sc, zp, axis, qlo, qhi = a
            x = np.maximum(x, np.float32(0)) if pre == "relu" else x
        assert (qlo, qhi) in ((-128, 127), (0, 255))
        return [O.fake_quant_qdq(x, sc, zp, axis=axis if sc.size > 1 else None, signed=qlo < 0)]
    return want


def _fq_set(a):
    xs, scs, zps, inner, qlo, qhi = a
    return [O.fake_quant_qdq(x, sc, zp, axis=1 if sc.size > 1 else None, signed=lo < 0) for x, sc, zp, lo in zip(xs, scs, zps, qlo)]


def _gptq(a):
    w, c0, nb, u, sc, zp, qlo, qhi, fmt = a
    W = w.copy()
    err = gptq_model.gptq_block(W, u, c0, nb, gptq_model.make_q({"fmt": fmt, "scale": sc, "zp": zp, "qlo": qlo, "qhi": qhi}))
    return [err], {0: W}


def _gptq_mx(a):
    w, c0, nb, u, elem = a
    W = w.copy()
    err, entry = mx_gptq_model.gptq_mx_block(W, u, c0, nb, elem, w.shape[1])
    scales = np.zeros((w.shape[0], -(-w.shape[1] // 32)), np.uint8)      # (a new tensor: zero outside the call's blocks)
    scales[:, c0 // 32:c0 // 32 + entry.shape[1]] = entry
    return [err, scales], {0: W}


def _no_near_tie(curve, best):
    """The searches pick the first minimum of an fp64 curve the device sums in another order (tests/test_hist_kl.py): a sample
    histogram whose two best candidates are further apart than that summation can move them has one answer."""
    others = np.delete(np.where(np.isnan(curve), np.inf, curve), best)
    assert others.min() > curve[best] * (1 + 1e-9) + 1e-300, "the sample histogram has a near tie: pick another"


def _kl(a):
    h, gmin, gmax, levels = a
    clip, best, curve = kl_model.kl_clip(h, np.float32(gmin), np.float32(gmax), levels)
    _no_near_tie(curve, best)
    return [clip]


def _qmse(a):
    h, gmin, gmax, qtype, bw, first = a
    clip, best, curve = qmse_model.qmse_clip(h, np.float32(gmin), np.float32(gmax), first, *qmse_model.grid_of(qtype, bw))
    _no_near_tie(curve, best)
    return [clip]


def _abs_hist(a):
    x, dmax, bins, hist = a
    return [], {3: hist + O.abs_hist(x.reshape(-1), bins, np.float32(dmax))}


# op -> numpy arguments -> [every output], or ([every output], {position of a mutated argument: what it holds afterwards})
DEFS = {
    "fake_quant": _fq(None),
    "fake_quant_relu": _fq("relu"),
    "fake_quant_add_relu": _fq("add_relu"),
    "fake_quant_set": _fq_set,
    "fake_quant_fp8": lambda a: [fp8_model.fake_quant_fp8(a[0], a[1], axis=a[2])],
    "fake_quant_mx": lambda a: [mx_model.fake_quant_mx(a[0], a[1], a[2])],
    "mx_encode": lambda a: list(P.encode(a[0], a[1], a[2])),
    "mx_decode": lambda a: [P.decode(a[0], a[1], a[2], a[3], a[4])],
    "mx_scale_search": lambda a: [S.scale_search(a[0], a[1], a[2])[0].reshape(T.block_shape(a[0].shape, a[1]))],
    "fake_quant_mx_scaled": lambda a: [S.fake_quant_mx_scaled(a[0], a[1], a[2], a[3])],
    "hadamard32": lambda a: [mx_rotate_model.fwht32(a[0])],
    "mx_gemm": lambda a: [G.mx_gemm(*a)[0]],
    "gptq_block": _gptq,
    "gptq_mx_block": _gptq_mx,
    "hist_kl": _kl,
    "hist_qmse": _qmse,
    "colwise_absmax": lambda a: [np.abs(a[0]).reshape(-1, a[0].shape[-1]).max(0)],
    # beyond the issue's table, from the oracle the other kernel tests use
    "minmax": lambda a: [np.array(O.minmax(a[0]), np.float32)],
    "rowwise_minmax": lambda a: [a[0].min(1), a[0].max(1)],
    "hist_percentile": lambda a: [np.asarray(O.hist_percentile(a[0], np.float32(a[1]), np.float32(a[2]), a[0].size, a[3]), np.float32)],
    "abs_hist_": _abs_hist,
}
VALUES_ONLY = ("mx_gemm",)


def test_every_op_of_the_issues_table_has_a_definition():
    for op in ("fake_quant", "fake_quant_relu", "fake_quant_add_relu", "fake_quant_set", "fake_quant_fp8", "fake_quant_mx", "mx_encode", "mx_decode",
               "mx_scale_search", "fake_quant_mx_scaled", "hadamard32", "mx_gemm", "gptq_block", "gptq_mx_block", "hist_kl", "hist_qmse",
               "colwise_absmax"):
        assert op in DEFS and op in T.CASES, op


# ------------------------------------------------------------------------------------------------ 1. real, fake, contiguous, definition
@pytest.mark.parametrize("op,case", T.all_cases(), ids=T.case_ids())
def test_real_op_against_fake_kernel_contiguous_self_and_definition(dev, op, case):
    args, kwargs = case.build(dev)
    before = _map(args, _host)
    real = outputs_of(_op(op)(*args, **kwargs))
    with FakeTensorMode():
        fargs, fkwargs = case.build(str(dev))
        fake = outputs_of(_op(op)(*fargs, **fkwargs))
    for (pos, t), (_, f) in zip(_tensors(args), _tensors(fargs)):       # the fake copies are copies: same geometry
        assert (t.shape, t.stride(), t.dtype, t.device) == (f.shape, f.stride(), f.dtype, f.device), (op, case.id, pos)
    assert len(real) == len(fake), (op, case.id, len(real), len(fake))
    for i, (r, f) in enumerate(zip(real, fake)):
        got = (tuple(r.shape), r.dtype, r.device, tuple(r.stride()))
        promised = (tuple(f.shape), f.dtype, f.device, tuple(f.stride()))
        assert got == promised, (op, case.id, i, got, promised)
    # the same call on contiguous copies of the same data
    cargs = _map(case.build(dev)[0], lambda t: t.contiguous())
    assert all(t.is_contiguous() for _, t in _tensors(cargs))
    contig = outputs_of(_op(op)(*cargs, **kwargs))
    if case.layout != "contig":
        assert any(not t.is_contiguous() for _, t in _tensors(args)), (op, case.id)
        for i, (r, c) in enumerate(zip(real, contig)):
            _same_bits(r, c, (op, case.id, "output", i, "against the op on x.contiguous()"))
        for (pos, t), (_, c) in zip(_tensors(args), _tensors(cargs)):       # mutated arguments too; the others are unchanged
            _same_bits(t, c, (op, case.id, "argument", pos, "after the call"))
    if op not in DEFS:
        return
    want = DEFS[op](list(before))
    want, mutated = want if isinstance(want, tuple) else (want, {})
    assert len(contig) == len(want), (op, case.id)
    for i, (c, w) in enumerate(zip(contig, want)):
        _same_as_definition(c, w, (op, case.id, "output", i, "against the definition"), values_only=op in VALUES_ONLY)
    for pos, w in mutated.items():
        _same_as_definition(cargs[pos], w, (op, case.id, "argument", pos, "against the definition"))
    for pos, t in _tensors(cargs):      # and nothing else was written
        if pos not in mutated:
            b = before[pos[0]][pos[1]] if isinstance(pos, tuple) else before[pos]
            _same_bits(t, b, (op, case.id, "argument", pos, "was written"))


# ------------------------------------------------------------------------------------------------ 2. opcheck
# op -> why test_aot_dispatch_dynamic is not run for it: a limit of the checker, never a defect of the op.  At most 5 of the 25.
AOT_DYNAMIC_EXCEPTIONS = {}
UTILS = ("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_dynamic")


def test_the_exception_list_is_short_and_names_ops():
    assert len(AOT_DYNAMIC_EXCEPTIONS) <= 5 and set(AOT_DYNAMIC_EXCEPTIONS) <= set(T.CASES)
    assert all(isinstance(why, str) and len(why) > 20 for why in AOT_DYNAMIC_EXCEPTIONS.values())


@pytest.mark.parametrize("op", sorted(T.CASES))
def test_opcheck(dev, op):
    cases = T.CASES[op]
    picked = [cases[0]] + [c for c in cases if c.layout != "contig"][:1]
    utils = tuple(u for u in UTILS if not (u == "test_aot_dispatch_dynamic" and op in AOT_DYNAMIC_EXCEPTIONS))
    try:
        for case in picked:
            args, kwargs = case.build(dev)
            outcome = torch.library.opcheck(_op(op).default, args, kwargs, test_utils=utils)
            assert set(outcome) == set(utils) and all(v == "SUCCESS" for v in outcome.values()), (op, case.id, outcome)
    finally:
        torch._dynamo.reset()


# ------------------------------------------------------------------------------------------------ 3. compiled graphs
def _compiled_equals_eager(fn, make_args, what, **compile_kw):
    """fn through torch.compile(aot_eager, fullgraph) on one set of new arguments, eagerly on another holding the same data: every
    result and every argument afterwards bit for bit.  -> seconds the first compiled call took (the compilation)."""
    compiled = torch.compile(fn, backend="aot_eager", fullgraph=True, **compile_kw)
    took = []
    for args_c, args_e in make_args:
        t0 = time.perf_counter()
        got = compiled(*args_c)
        torch.cuda.synchronize()
        took.append(time.perf_counter() - t0)
        want = fn(*args_e)
        got, want = outputs_of(got), outputs_of(want)
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            assert tuple(g.shape) == tuple(w.shape) and g.dtype == w.dtype and tuple(g.stride()) == tuple(w.stride()), (what, i)
            _same_bits(g, w, (what, "result", i))
        for i, (a, b) in enumerate(zip(args_c, args_e)):
            _same_bits(a, b, (what, "argument", i))
    print(f"torch.compile {what}: calls took {', '.join(f'{t:.2f} s' for t in took)}")
    return took


def _dev(a, dev, layout="contig"):
    return T.place(a, dev, layout)


def test_compiled_transposed_activation_through_add_relu_and_per_channel_pair(dev):
    """(a) a transposed activation -> fake_quant_add_relu -> .t() -> fake_quant per channel."""
    rng = np.random.default_rng(1)
    x, x2 = (rng.standard_normal((6, 8)) * 3).astype(np.float32), (rng.standard_normal((6, 8)) * 3).astype(np.float32)
    sc, zp, qlo, qhi = T.fq_params((8, 6), 0, False, "compiled")

    def fn(x, x2, sc1, zp1, scc, zpc):
        y = torch.ops.dipoorlet.fake_quant_add_relu(x, x2, sc1, zp1, 0, -128, 127)
        return torch.ops.dipoorlet.fake_quant(y.t(), scc, zpc, 0, qlo, qhi)

    def args():
        return (_dev(x, dev, "t2d"), _dev(x2, dev, "t2d"), _dev(np.array([0.05], np.float32), dev), _dev(np.array([-5], np.int32), dev),
                _dev(sc, dev), _dev(zp, dev))
    try:
        _compiled_equals_eager(fn, [(args(), args())], "(a) add_relu -> t() -> per-channel pair")
        mid = O.fake_quant_qdq(np.maximum(x + x2, np.float32(0)), np.float32(0.05), -5)
        _same_as_definition(fn(*args()), O.fake_quant_qdq(mid.T, sc, zp, axis=0, signed=False), "(a) against the oracle")
    finally:
        torch._dynamo.reset()


def test_compiled_rotate_encode_gemm_fp8_under_dynamic_shapes(dev):
    """(b) hadamard32 -> mx_encode -> mx_gemm against a packed constant -> fake_quant_fp8, compiled once with dynamic=True and run
    at K = 32 and at K = 40 (the block axis is axis 0 of the rotated [K, 32] activation: Kp = 32 and 64)."""
    rng = np.random.default_rng(2)

    def fn(x, w_codes, w_scales, sc):
        r = torch.ops.dipoorlet.hadamard32(x)
        a_codes, a_scales = torch.ops.dipoorlet.mx_encode(r, 0, "mxfp8")
        c = torch.ops.dipoorlet.mx_gemm(a_codes, a_scales, w_codes, w_scales, "mxfp8", "mxfp4")
        return torch.ops.dipoorlet.fake_quant_fp8(c, sc, 0)
    runs = []
    for k in (32, 40):
        x = rng.standard_normal((k, 32)).astype(np.float32)
        wc, ws = P.encode(rng.standard_normal((k, 9)).astype(np.float32), 0, "mxfp4")      # a [K, N] weight packed along K: [N, Kp / 2]

        def args(x=x, wc=wc, ws=ws):
            return (_dev(x, dev), _dev(wc, dev), _dev(ws, dev), _dev(np.array([0.37], np.float32), dev))
        runs.append((args(), args()))
    try:
        _compiled_equals_eager(fn, runs, "(b) hadamard32 -> mx_encode -> mx_gemm -> fake_quant_fp8, K = 32 then 40", dynamic=True)
        for (a, _), k in zip(runs, (32, 40)):
            assert tuple(fn(*a).shape) == (32, 9), k
    finally:
        torch._dynamo.reset()


def test_compiled_range_histogram_percentile_over_two_tensors(dev):
    """(c) minmax_batched -> abs_hist_batched_ -> hist_percentile on two tensors: the mutated mins, maxs and hist are checked."""
    rng = np.random.default_rng(3)
    xs = [rng.standard_normal((4, 50)).astype(np.float32), (rng.standard_normal((2, 3, 5, 5)) * 2).astype(np.float32)]

    def fn(x0, x1, mins, maxs, hist):
        torch.ops.dipoorlet.minmax_batched([x0, x1], mins, maxs)
        torch.ops.dipoorlet.abs_hist_batched_([x0, x1], mins, maxs, 64, hist)
        return torch.ops.dipoorlet.hist_percentile(hist[1], -8.0, 8.0, 0.99)

    def args():
        return (_dev(xs[0], dev), _dev(xs[1], dev), _dev(np.full(2, np.inf, np.float32), dev), _dev(np.full(2, -np.inf, np.float32), dev),
                _dev(np.zeros((2, 64), np.int64), dev))
    try:
        a = args()
        _compiled_equals_eager(fn, [(a, args())], "(c) minmax_batched -> abs_hist_batched_ -> hist_percentile")
        assert _host(a[2]).tolist() == [float(x.min()) for x in xs] and _host(a[3]).tolist() == [float(x.max()) for x in xs]
        for t, x in enumerate(xs):
            assert np.array_equal(_host(a[4])[t], O.abs_hist(x.reshape(-1), 64, O.hist_dmax(x.min(), x.max()))), t
    finally:
        torch._dynamo.reset()


def test_compiled_gptq_block_in_place_then_a_read_of_w(dev):
    """(d) gptq_block mutating w in place, followed by a read of w."""
    w = T._normal((5, 40), "compiled w", spread=1.0)
    u = T.gptq_factor(40, 5)
    sc, zp, qlo, qhi = T.fq_params((5, 40), 0, False, "compiled gptq")

    def fn(w, u, sc, zp):
        err = torch.ops.dipoorlet.gptq_block(w, 8, 16, u, sc, zp, qlo, qhi, "int")
        return err, w * 2.0

    def args():
        return (_dev(w, dev), _dev(u, dev), _dev(sc, dev), _dev(zp, dev))
    try:
        a = args()
        _compiled_equals_eager(fn, [(a, args())], "(d) gptq_block in place -> w * 2")
        W = w.copy()
        gptq_model.gptq_block(W, u, 8, 16, gptq_model.make_q({"fmt": "int", "scale": sc, "zp": zp, "qlo": qlo, "qhi": qhi}))
        _same_as_definition(a[0], W, "(d) w against the model")
        assert not np.array_equal(W, w)
    finally:
        torch._dynamo.reset()
