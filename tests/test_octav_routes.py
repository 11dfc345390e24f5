"""The OCTAV pairs that neither the streaming walk nor the rescue finish — values of 2^14 and above or +-inf, a log bin of 2^20
values or more, a pair the rescue walk gives up on — take the compaction route.  Every entry point must return FINAL rows for them:
the custom ops (torch.ops.dipoorlet.octav / octav_batched) as soon as the caller's stream reaches them, without a pipeline sync() —
against the fp64 numpy oracle (forward_net.py:315-330), on cold plans, on the default and on a pool stream, unchanged after more
calls of the same geometry, and holding no reference to their inputs; ops.octav_batch in all four forms and OctavPipeline (after
sync()) on the 2^20-bin pairs."""
import warnings

import numpy as np
import pytest
import torch

from dipoorlet_amd import _hip, ops, torch_ops
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
B = 3
N = 25088
BIG = 2 ** 20 + 1               # a constant pair: one log bin of 2^20 + 1 values
HUGE = 3 * 2 ** 20              # almost all values equal
# (kind, elements per image): ordinary pairs next to every trigger of the compaction route, and NaN (a fixed point: no route)
ROUTES = (("normal", N), ("relu", N), ("p2_14", N), ("v20000", N), ("pinf", N), ("ninf", N), ("nan", N), ("const", BIG),
          ("near_const", HUGE))
SET = (("normal", 25088), ("relu", 150528), ("laplace", 1000), ("uniform", 2048), ("spike", 25088), ("tiny", 2048))
CHECKED = 3                     # calls whose rows are compared with the oracle; the calls behind them only push the plan on
CALLS = 7                       # more than the default three pipeline sets: a deferred settle would have fired


def _close(a, b, tol=TOL):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        return np.all(both_nan | (a == b) | (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))   # (a == b: equal infinities)


def _route_pair(kind, n, rng):
    if kind == "const":
        return np.full(n, 0.37, np.float32)
    if kind == "near_const":
        x = np.full(n, 0.37, np.float32)
        x[rng.integers(0, n, 1000)] = rng.standard_normal(1000).astype(np.float32)
        return x
    x = rng.standard_normal(n).astype(np.float32) * 2
    if kind == "relu":
        return np.maximum(x, np.float32(0))
    at = rng.integers(0, n)
    x[at] = {"normal": x[at], "p2_14": 2.0 ** 14, "v20000": 20000.0, "pinf": np.inf, "ninf": -np.inf, "nan": np.nan}[kind]
    return x


def _sets(kinds, count, seed, make=None):
    """`count` batches of the tensor set `kinds`: (host [B, n] arrays, device tensors) each."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        if make is None:
            host = [np.stack([_route_pair(k, n, rng) for _ in range(B)]) for k, n in kinds]
        else:
            host = [np.stack([make(k, n, int(rng.integers(1 << 30))) for _ in range(B)]) for k, n in kinds]
        out.append((host, [torch.from_numpy(h).cuda() for h in host]))
    return out


def _oracle(host, dyn):
    """[B, T, 3] fp64: (s, min, max) of every pair of one batch."""
    want = np.zeros((B, len(host), 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for t, h in enumerate(host):
            for b in range(B):
                mn, mx = O.minmax(h[b])
                want[b, t] = (O.octav_scale(h[b], O.octav_unsigned(mn, dyn)), mn, mx)
    return want


def _check(got, want, what):
    got = np.asarray(got)
    assert np.array_equal(got[..., 1:], want[..., 1:].astype(np.float32), equal_nan=True), (what, got[..., 1:], want[..., 1:])
    bad = [i for i in np.ndindex(got.shape[:-1]) if not _close(got[i + (0,)], want[i + (0,)])]
    assert not bad, (what, [(i, float(got[i + (0,)]), float(want[i + (0,)])) for i in bad[:8]])


@pytest.fixture(scope="module")
def route_sets():
    assert torch.cuda.is_available(), "needs the MI355X"
    sets = _sets(ROUTES, CALLS, 91)
    want = {dyn: [_oracle(h, dyn) for h, _ in sets[:CHECKED]] for dyn in (False, True)}
    return sets, want


@pytest.fixture
def cold(monkeypatch):
    """The custom ops' plan cache, empty: every geometry's first call builds its plan (the OCTAV workspace included)."""
    monkeypatch.setattr(torch_ops, "_PLANS", {})


def _calls_are_final(call, inputs, want, stream, what):
    """call(inputs[0]) .. call(inputs[-1]) on `stream` (None: the current stream); the rows of the first CHECKED calls against
    `want`, read as a torch caller reads them — behind the stream, never after a pipeline sync() —, and call 1's rows read again
    after all the others: bit for bit what they were."""
    assert len(inputs) > ops._PIPE_SETS + 1

    def sync():
        (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()            # (the inputs are the default stream's work)
    with torch.cuda.stream(stream):     # (None: the current stream)
        outs = [call(inputs[0])]
        sync()
        first = outs[0].cpu().numpy().copy()
        _check(first, want[0], (what, 0))
        for k in range(1, CHECKED):
            outs.append(call(inputs[k]))
            sync()
            _check(outs[k].cpu().numpy(), want[k], (what, k))
        for x in inputs[CHECKED:]:
            outs.append(call(x))
        sync()
        again = outs[0].cpu().numpy()
    assert again.view(np.uint32).tobytes() == first.view(np.uint32).tobytes(), (what, "call 1 changed", first, again)


@pytest.mark.parametrize("on_pool_stream", [False, True], ids=["current_stream", "pool_stream"])
@pytest.mark.parametrize("dyn", [False, True], ids=["asym", "dynamic_sym"])
def test_octav_batched_route_pairs_are_final(route_sets, cold, dyn, on_pool_stream):
    """octav_batched over B = 3 images of a set that mixes ordinary pairs with every trigger of the compaction route."""
    sets, want = route_sets
    stream = torch.cuda.Stream() if on_pool_stream else None
    _calls_are_final(lambda xs: torch.ops.dipoorlet.octav_batched(xs, dyn), [dev for _, dev in sets], want[dyn], stream,
                     ("octav_batched", dyn))


@pytest.mark.parametrize("on_pool_stream", [False, True], ids=["current_stream", "pool_stream"])
@pytest.mark.parametrize("dyn", [False, True], ids=["asym", "dynamic_sym"])
def test_octav_per_tensor_route_pairs_are_final(route_sets, cold, dyn, on_pool_stream):
    """octav per tensor: each pair kind on a cold plan (seven of them share one geometry: the cache is emptied between kinds)."""
    sets, want = route_sets
    stream = torch.cuda.Stream() if on_pool_stream else None
    for t, (kind, _) in enumerate(ROUTES):
        torch_ops._PLANS.clear()        # (the fixture's dict)
        # the same pair of every batch, images in turn: CALLS calls of one geometry
        inputs = [sets[k][1][t][k % B] for k in range(CALLS)]
        rows = [want[dyn][k][k % B, t][None, None] for k in range(CHECKED)]
        _calls_are_final(lambda x: torch.ops.dipoorlet.octav(x, dyn).view(1, 1, 3), inputs, rows, stream, ("octav", kind, dyn))


@pytest.mark.parametrize("dyn", [False, True], ids=["asym", "dynamic_sym"])
def test_octav_ops_rescue_refused_pairs_are_final(cold, dyn):
    """Ordinary data whose walks are refused for every second pair, and the rescue walk too (the C ABI's test hooks): those pairs
    finish on the compaction route."""
    from _cases import make_tensor
    sets = _sets(SET, CALLS, 17, make=make_tensor)
    want = [_oracle(h, dyn) for h, _ in sets[:CHECKED]]
    L = _hip.lib()
    old = (L.dpl_test_hook_exact_fail_every(2), L.dpl_test_hook_rescue_fail_every(2))
    try:
        _calls_are_final(lambda xs: torch.ops.dipoorlet.octav_batched(xs, dyn), [dev for _, dev in sets], want, None,
                         ("octav_batched", dyn))
        t = 1       # (150 528 elements: a pair the per-tensor plan walks on its own)
        _calls_are_final(lambda x: torch.ops.dipoorlet.octav(x, dyn).view(1, 1, 3), [sets[k][1][t][0] for k in range(CALLS)],
                         [want[k][0, t][None, None] for k in range(CHECKED)], None, ("octav", dyn))
    finally:
        L.dpl_test_hook_exact_fail_every(old[0])
        L.dpl_test_hook_rescue_fail_every(old[1])


def test_octav_ops_keep_no_reference_to_their_inputs(route_sets):
    """After a warm call, an OCTAV op's inputs and its output, once the caller drops them, are the allocator's again: the op keeps
    nothing of them (the device memory in use returns to what it was before the inputs existed).  The warm call runs on tensors
    the fixture keeps alive anyway, so that an op holding on to its last call's inputs cannot hide them in `before`."""
    sets, _ = route_sets
    for op, live in ((lambda xs: torch.ops.dipoorlet.octav_batched(xs, False), sets[0][1]),
                     (lambda xs: torch.ops.dipoorlet.octav(xs[0], True), [sets[0][1][8][1]])):
        op(live)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        xs = [x.clone() for x in live]
        out = op(xs)
        del xs, out
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before


# the other entry points on the 2^20-bin trigger: what the CLI and bench.py run
BIN_SET = (("normal", 25088), ("const", BIG), ("relu", 150528), ("near_const", HUGE))


@pytest.fixture(scope="module")
def bin_sets():
    assert torch.cuda.is_available(), "needs the MI355X"
    sets = _sets(BIN_SET, 3, 57)
    return sets, {dyn: [_oracle(h, dyn) for h, _ in sets] for dyn in (False, True)}


@pytest.mark.parametrize("form", ["tail", "bracket", "compact", "full"])
def test_octav_batch_bin_of_2_20_values(bin_sets, form):
    sets, want = bin_sets
    elems = [n for _, n in BIN_SET]
    for dyn in (False, True):
        plan = ops.TensorSetPlan(elems, B, torch.device("cuda:0"))
        for k, (_, dev) in enumerate(sets):
            _check(ops.octav_batch(plan, dev, dyn, form=form).cpu().numpy(), want[dyn][k], (form, dyn, k))


@pytest.mark.parametrize("lanes", [1, 2])
def test_octav_pipeline_bin_of_2_20_values(bin_sets, monkeypatch, lanes):
    monkeypatch.setenv("DPL_OCTAV_FORM", "tail")
    sets, want = bin_sets
    elems = [n for _, n in BIN_SET]
    for dyn in (False, True):
        plan = ops.TensorSetPlan(elems, B, torch.device("cuda:0"))
        pipe = ops.OctavPipeline(dyn, lanes=lanes)
        outs = [pipe.submit(plan, dev) for _, dev in sets + sets[:1]]
        pipe.sync()
        torch.cuda.synchronize()
        assert pipe.compaction_pairs >= B * len(outs)       # (the constant pair of every image, at least)
        for k, o in enumerate(outs):
            _check(o.cpu().numpy(), want[dyn][k % len(sets)], (lanes, dyn, k))
