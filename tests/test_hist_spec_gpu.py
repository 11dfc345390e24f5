"""GPU: the range pass's histogram speculation (CalibAccumulators over BoundSets; csrc/calib_kernels.hip K2s) against the model
(tests/hist_spec_model.py), against the same calls on plain lists of tensors (which never speculate) and against the numpy oracle.

Every result is compared for EQUALITY: the speculation may only ever skip work.  Every test that expects speculation also proves
that it RAN — the device's skip flags equal the model's table, which is known in advance because the inputs are built so that each
tensor takes its extreme in a chosen batch — so a silent fall-back to the plain path cannot pass.
"""
import numpy as np
import pytest

import torch

import hist_spec_model as M
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

K = 5       # batches per shard
B = 2       # images per batch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    from dipoorlet_amd import _hip
    st, name, _, _ = _hip.device_info()
    assert st == 0, name
    return torch.device("cuda:0")


# ---- inputs whose table is known in advance ------------------------------------------------------------------------------------
# (name, elements per image, kind, peak, batches that hold the peak)
def _spec(big):
    return [("relu_first", big, "relu", 6.0, (0,)),
            ("signed_min_last", 70001, "signed_min", 9.5, (K - 1,)),
            ("relu_middle", 65536, "relu", 4.25, (2,)),
            ("signed_tie", 50000, "signed", 3.0, (1, 3)),
            ("all_zero", 4099, "zero", 0.0, ()),
            ("neg_zero_max", 30001, "nonpos", 2.5, (0,)),
            ("tiny", 3, "signed", 1.5, (1,)),
            ("unaligned", 123457, "relu", 7.75, (3,)),
            ("exact_div", 20000, "relu", 1e-33, (0,)),
            ("one", 1, "signed", 2.0, (2,))]


def _make_batches(spec, seed, k_batches=K, batch=B):
    """-> batches[k][t]: float32 numpy [batch, elems]; |values| <= 0.8 peak except the planted peak in its batches."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(k_batches):
        row = []
        for name, e, kind, peak, where in spec:
            n = batch * e
            if kind == "zero":
                x = np.zeros(n, np.float32)
            else:
                x = np.clip(rng.standard_normal(n) * 0.25, -0.8, 0.8).astype(np.float32) * np.float32(peak)
                if kind == "relu":
                    x = np.maximum(x, 0)
                elif kind == "nonpos":
                    x = -np.abs(x)
                    x[x == 0] = np.float32(-0.0)
                    x[0] = np.float32(-0.0)         # the maximum of every batch is -0.0
                pos = int(rng.integers(1 if kind == "nonpos" and n > 1 else 0, n))
                if k in where:
                    x[pos] = np.float32(-peak if kind in ("signed_min", "nonpos") else peak)
                elif kind in ("signed_min",):
                    x[pos] = np.float32(-0.85 * peak)       # dmax comes from the minimum in every batch
            row.append(x.reshape(batch, e))
        out.append(row)
    return out


def _batch_dmax(batches):
    d = np.zeros((len(batches), len(batches[0])), np.float32)
    for k, row in enumerate(batches):
        for t, x in enumerate(row):
            lo, hi = O.minmax(x)
            d[k, t] = O.hist_dmax(lo, hi)
    return d


def _range_ok(dmax, bins):
    ok = []
    for d in dmax:
        try:
            np.histogram(np.zeros(1, np.float32), bins, (0, np.float32(d)))
            ok.append(True)
        except ValueError:
            ok.append(False)
    return ok


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _results(acc):
    out = {"hist": acc.hist.clone(), "gmin": acc.gmin.clone(), "gmax": acc.gmax.clone(), "clip": acc.hist_percentile(0.99999)}
    if acc.bins >= 2:
        clip, best, div = acc.hist_kl(min(128, acc.bins))
        out.update(kl_clip=clip, kl_best=best, kl_div=div)
    return out


def _assert_same_results(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert _same(a[key], b[key]), key


def _sweep(acc, p1, p2=None, merged=None):
    """bench.py's sequence: p1 = [(plan, tensors)] of the range pass, p2 of the histogram pass (default: the same);
    merged(gmin, gmax) -> ranges to install with set_minmax."""
    acc.reset_minmax()
    for plan, x in p1:
        acc.minmax_accumulate(plan, x)
    gmin, gmax = acc.finalize_minmax()
    if merged is not None:
        acc.set_minmax(*merged(gmin.clone(), gmax.clone()))
    acc.hist_prepare()
    for plan, x in (p1 if p2 is None else p2):
        acc.abs_hist_accumulate(plan, x)
    return _results(acc)


def _upload(batches, dev):
    return [[torch.from_numpy(x).to(dev) for x in row] for row in batches]


def _case(dev, bins, seed=0, speculate=True, scale=1):
    from dipoorlet_amd import ops
    # the first tensor is sized so that an entry (T * bins * 4 B) stays below 1/64 of the batch's bytes
    spec = _spec(max(100003, scale * 64 * 10 * bins // B + 1001))
    batches = _make_batches(spec, seed)
    elems = [e for _, e, _, _, _ in spec]
    plan = ops.TensorSetPlan(elems, B, dev)
    acc = ops.CalibAccumulators(len(elems), dev, bins, speculate=speculate)
    return ops, spec, batches, elems, plan, acc


def acc_range_flags(plan, batches, dev, bins):
    """exact_div of every tensor's final range, from the plain path."""
    from dipoorlet_amd import ops
    a = ops.CalibAccumulators(plan.T, dev, bins)
    for row in batches:
        a.minmax_accumulate(plan, [torch.from_numpy(x).to(dev) for x in row])
    a.finalize_minmax()
    a.hist_prepare()
    return a.range_status()["exact_div"]


def _assert_oracle(hist, rows, bins, fin, tensors):
    """hist[t] equals np.histogram's counts (oracle.np_oracle.abs_hist) over the batches `rows` of the histogram pass, bit for bit."""
    for t in tensors:
        x = np.concatenate([row[t].ravel() for row in rows])
        assert np.array_equal(hist[t].cpu().numpy(), O.abs_hist(x, bins, fin[t])), t


def _flags(acc, bound):
    return [acc.spec_flags(x).numpy() for x in bound]


@pytest.mark.parametrize("bins", [2048, 1, 1000, 16384])
def test_flags_equal_the_model_and_results_equal_the_plain_path(dev, bins):
    """ReLU and signed tensors, dmax from the minimum, an all-zero tensor (the degenerate +-0.5 range: the exact-divide path in the
    fused kernel), -0.0 maxima, a range so small that the index estimate needs the exact divide, tiny and unaligned tensors; extremes
    in the first, a middle, the last batch and in two batches with equal dmax.  Required share of pairs skipped: the model's table
    for these inputs — (K - 1) + 0 + 2 + 3 + (K - 1) + (K - 1) + 3 + 1 + (K - 1) + 2 = 27 of 50 at K = 5."""
    ops, spec, batches, elems, plan, acc = _case(dev, bins)
    dmax = _batch_dmax(batches)
    fin = dmax.max(0)
    valid = M.valid_table(dmax, fin, _range_ok(fin, bins))
    ok = np.array(_range_ok(fin, bins))
    expect = [(K - 1), 0, 2, 3, (K - 1), (K - 1), 3, 1, (K - 1), 2]
    assert [int(valid[:, t].sum()) if ok[t] else 0 for t in range(len(spec))] == [e if ok[t] else 0 for t, e in enumerate(expect)]
    assert ok.all(), "the constructed ranges must be ones numpy accepts"
    assert acc_range_flags(plan, batches, dev, bins)[8] == 1, "the tiny range must take the exact-divide path"
    xs = _upload(batches, dev)
    bound = [plan.bind(row) for row in xs]
    assert all(acc.will_speculate(plan, x) for x in bound)
    got = _sweep(acc, [(plan, x) for x in bound])
    flags = np.stack(_flags(acc, bound))
    print("skipped pairs per tensor:", (flags == 1).sum(0).tolist(), "model:", valid.sum(0).tolist())
    assert np.array_equal(flags == 1, valid), "the device's skip flags differ from the model's table"
    assert np.array_equal(flags == 2, np.broadcast_to(~ok, flags.shape))
    st = acc.spec_stats()
    e_batch = np.array(elems, np.int64) * B
    assert st["pairs"] == K * len(spec) and st["pairs_skipped"] == int(valid.sum())
    assert st["elements"] == K * int(e_batch.sum()) and st["elements_skipped"] == int((valid * e_batch[None, :]).sum())
    # ... the unspeculated path: the same calls on plain lists
    ref_acc = ops.CalibAccumulators(len(elems), dev, bins)
    ref = _sweep(ref_acc, [(plan, row) for row in xs])
    assert ref_acc.spec_stats()["pairs"] == 0
    _assert_same_results(got, ref)
    # ... numpy on a sample of tensors (all batches of the shard)
    for t in (1, 3, 4, 5, 6, 7, 9):
        x = np.concatenate([row[t].ravel() for row in batches])
        assert np.array_equal(got["hist"][t].cpu().numpy(), O.abs_hist(x, bins, fin[t])), spec[t][0]
    # ... and the cuts of the remaining stream, for the last batch's flags
    cuts = acc.spec_cuts(plan, bound[-1]).numpy().tolist()
    assert cuts == M.cuts(e_batch.tolist(), (flags[-1] != 0).tolist(), plan.work("hist").n_blocks)


@pytest.mark.parametrize("n_tensors", [2048, 2049])
def test_the_largest_set_that_speculates_and_the_first_that_does_not(dev, n_tensors):
    """_hip.HIST_SPEC_MAX_TENSORS = 2048 tensors: the largest P[n_tensors + 1] k_abs_hist_rest and k_hist_spec_cuts keep in LDS.
    Per-image sizes 1024 + (t mod 7), B = 2, three batches, 16 bins: a batch is 16.8 MB, an entry's T * bins * 4 * 64 = 8.4 MB stays
    below it, so the set speculates; extremes planted in batch t mod 3, so a third of the tensors is still read in the last batch and
    the rest skipped.  One tensor more does not speculate.  Both: the BoundSet sweep == the plain-list sweep == numpy."""
    from dipoorlet_amd import _hip, ops
    assert _hip.HIST_SPEC_MAX_TENSORS == 2048
    bins, n_batches = 16, 3
    kinds = ("relu", "signed", "signed_min")
    spec = [("t%d" % t, 1024 + t % 7, kinds[t % 5 % 3], 1.0 + 0.125 * (t % 11), (t % 3,)) for t in range(n_tensors)]
    batches = _make_batches(spec, 17, k_batches=n_batches)
    elems = [e for _, e, _, _, _ in spec]
    plan = ops.TensorSetPlan(elems, B, dev)
    acc = ops.CalibAccumulators(n_tensors, dev, bins)
    dmax = _batch_dmax(batches)
    fin = dmax.max(0)
    ok = _range_ok(fin, bins)
    assert all(ok)
    valid = M.valid_table(dmax, fin, ok)
    assert [int(valid[:, t].sum()) for t in range(6)] == [2, 1, 0, 2, 1, 0], "extremes in batch t mod 3"
    xs = _upload(batches, dev)
    bound = [plan.bind(row) for row in xs]
    speculates = n_tensors <= 2048
    assert n_tensors * bins * 4 * acc.SPEC_MAX_SHARE <= plan.total * 4
    assert all(acc.will_speculate(plan, x) == speculates for x in bound)
    got = _sweep(acc, [(plan, x) for x in bound])
    st = acc.spec_stats()
    if speculates:
        flags = np.stack(_flags(acc, bound))
        assert np.array_equal(flags == 1, valid), "the device's skip flags differ from the model's table"
        assert not (flags == 2).any()
        assert st["pairs"] == n_batches * n_tensors and st["pairs_skipped"] == int(valid.sum())
        e_batch = np.array(elems, np.int64) * B
        assert st["elements_skipped"] == int((valid * e_batch[None, :]).sum())
        cuts = acc.spec_cuts(plan, bound[-1]).numpy().tolist()
        assert cuts == M.cuts(e_batch.tolist(), (flags[-1] != 0).tolist(), plan.work("hist").n_blocks)
    else:
        assert st["pairs"] == 0 and not acc._ledger and acc.spec_flags(bound[0]) is None and acc.spec_cuts(plan, bound[-1]) is None
    ref_acc = ops.CalibAccumulators(n_tensors, dev, bins)
    ref = _sweep(ref_acc, [(plan, row) for row in xs])
    assert ref_acc.spec_stats()["pairs"] == 0
    _assert_same_results(got, ref)
    _assert_oracle(got["hist"], batches, bins, fin, list(range(0, n_tensors, 97)) + [2046, 2047, n_tensors - 1])


@pytest.mark.parametrize("when", [0, 2, K - 1])
def test_nan_in_the_first_a_middle_and_the_last_batch(dev, when):
    """A NaN makes the tensor's range NaN (status 1: numpy raises): nothing of it is counted on either path, and from the batch
    behind the NaN on the range pass has no guess for it.  The other tensors are skipped as the model says."""
    ops, spec, batches, elems, plan, acc = _case(dev, 2048, seed=3)
    batches[when][0][1, 77] = np.nan
    batches[when][3][0, 5] = np.nan
    dmax = _batch_dmax(batches)
    with np.errstate(invalid="ignore"):
        fin = np.where(np.isnan(dmax).any(0), np.float32(np.nan), dmax.max(0)).astype(np.float32)
    valid = M.valid_table(dmax, fin, _range_ok(np.nan_to_num(fin), 2048))
    assert not valid[:, 0].any() and not valid[:, 3].any() and valid.sum() == 27 - (K - 1) - 3
    xs = _upload(batches, dev)
    bound = [plan.bind(row) for row in xs]
    got = _sweep(acc, [(plan, x) for x in bound])
    flags = np.stack(_flags(acc, bound))
    assert np.array_equal(flags == 1, valid)
    assert (flags[:, 0] == 2).all() and (flags[:, 3] == 2).all()
    assert acc.range_status()["status"][0] == 1 and int(got["hist"][0].sum()) == 0
    ref = _sweep(ops.CalibAccumulators(len(elems), dev, 2048), [(plan, row) for row in xs])
    _assert_same_results(got, ref)
    _assert_oracle(got["hist"], batches, 2048, fin, (1, 2, 4, 5, 6, 7, 9))      # (the tensors without a NaN)


def test_merged_ranges_decide_by_the_same_comparison(dev):
    """set_minmax between the passes (several ranks): a larger merged range invalidates every guess — everything is read, the
    counts are those of the plain path —; the unchanged range leaves the model's table."""
    ops, spec, batches, elems, plan, acc = _case(dev, 2048, seed=5)
    dmax = _batch_dmax(batches)
    xs = _upload(batches, dev)
    bound = [plan.bind(row) for row in xs]
    larger = lambda lo, hi: (lo * 2 - 1, hi * 2 + 1)                            # noqa: E731
    got = _sweep(acc, [(plan, x) for x in bound], merged=larger)
    assert not np.stack(_flags(acc, bound)).any() and acc.spec_stats(reset=True)["pairs_skipped"] == 0
    ref = _sweep(ops.CalibAccumulators(len(elems), dev, 2048), [(plan, row) for row in xs], merged=larger)
    _assert_same_results(got, ref)
    x = np.concatenate([row[0].ravel() for row in batches])
    assert np.array_equal(got["hist"][0].cpu().numpy(), O.abs_hist(x, 2048, np.float32(2 * 6.0 + 1)))
    got = _sweep(acc, [(plan, x) for x in bound], merged=lambda lo, hi: (lo, hi))
    fin = dmax.max(0)
    valid = M.valid_table(dmax, fin, _range_ok(fin, 2048))
    assert np.array_equal(np.stack(_flags(acc, bound)) == 1, valid) and acc.spec_stats()["pairs_skipped"] == int(valid.sum())
    ref = _sweep(ops.CalibAccumulators(len(elems), dev, 2048), [(plan, row) for row in xs], merged=lambda lo, hi: (lo, hi))
    _assert_same_results(got, ref)


def test_ragged_last_batch_through_a_second_plan(dev):
    ops, spec, batches, elems, plan, acc = _case(dev, 2048, seed=7, scale=2)
    tail = _make_batches(spec, 70, k_batches=1, batch=1)
    plan1 = ops.TensorSetPlan(elems, 1, dev)
    # (the set is sized so that the one-image plan's batch, half as many bytes, still carries an entry)
    xs, xt = _upload(batches, dev), _upload(tail, dev)
    bound = [plan.bind(row) for row in xs]
    bt = plan1.bind(xt[0])
    seq = [(plan, x) for x in bound] + [(plan1, bt)]
    got = _sweep(acc, seq)
    dmax = np.concatenate([_batch_dmax(batches), _batch_dmax(tail)])
    fin = dmax.max(0)
    valid = M.valid_table(dmax, fin, _range_ok(fin, 2048))
    flags = np.stack(_flags(acc, bound))
    assert np.array_equal(flags == 1, valid[:K])
    assert acc.will_speculate(plan1, bt)
    assert np.array_equal(acc.spec_flags(bt).numpy() == 1, valid[K]) and valid[K].sum() >= 5
    ref = _sweep(ops.CalibAccumulators(len(elems), dev, 2048), [(plan, row) for row in xs] + [(plan1, xt[0])])
    _assert_same_results(got, ref)
    for t in (0, 2, 7):
        x = np.concatenate([row[t].ravel() for row in batches] + [tail[0][t].ravel()])
        assert np.array_equal(got["hist"][t].cpu().numpy(), O.abs_hist(x, 2048, fin[t]))


def test_a_set_seen_twice_and_the_histogram_pass_out_of_order(dev):
    """Range pass over A B A C: A's entry is the one of its second visit (the latest wins).  Histogram pass over C A B A A: a set
    may come in any order and any number of times; every call adds that batch's histogram."""
    ops, spec, batches, elems, plan, acc = _case(dev, 2048, seed=9)
    xs = _upload(batches[:3], dev)
    A, Bs, Cs = [plan.bind(row) for row in xs]
    p1 = [(plan, A), (plan, Bs), (plan, A), (plan, Cs)]
    p2 = [(plan, Cs), (plan, A), (plan, Bs), (plan, A), (plan, A)]
    got = _sweep(acc, p1, p2)
    d3 = _batch_dmax(batches[:3])
    dmax = d3[[0, 1, 0, 2]]
    fin = dmax.max(0)
    valid = M.valid_table(dmax, fin, _range_ok(fin, 2048))
    assert np.array_equal(acc.spec_flags(A).numpy() == 1, valid[2])
    assert np.array_equal(acc.spec_flags(Bs).numpy() == 1, valid[1])
    assert np.array_equal(acc.spec_flags(Cs).numpy() == 1, valid[3])
    assert valid[2].sum() > valid[0].sum(), "the second visit of A comes behind the batches that hold the extremes"
    assert acc.spec_stats()["pairs_skipped"] == int(valid[3].sum() + 3 * valid[2].sum() + valid[1].sum())
    lists = {id(A): xs[0], id(Bs): xs[1], id(Cs): xs[2]}
    ref = _sweep(ops.CalibAccumulators(len(elems), dev, 2048), [(p, lists[id(x)]) for p, x in p1], [(p, lists[id(x)]) for p, x in p2])
    _assert_same_results(got, ref)
    _assert_oracle(got["hist"], [batches[i] for i in (2, 0, 1, 0, 0)], 2048, fin, (1, 2, 3, 5, 7, 9))
    # twice doubles
    h1 = acc.hist.clone()
    for p, x in p2:
        acc.abs_hist_accumulate(p, x)
    assert torch.equal(acc.hist, 2 * h1)


def test_reset_between_sweeps_and_the_slab_is_reused(dev):
    ops, spec, batches, elems, plan, acc = _case(dev, 2048, seed=11)
    xs = _upload(batches, dev)
    bound = [plan.bind(row) for row in xs]
    seq = [(plan, x) for x in bound]
    first = _sweep(acc, seq)
    f1 = np.stack(_flags(acc, bound))
    entries = sorted(rec[1].data_ptr() for rec in acc._ledger.values())
    acc.reset_minmax()
    assert not acc._ledger and acc.spec_flags(bound[0]) is None, "reset_minmax empties the ledger"
    second = _sweep(acc, seq)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    third = _sweep(acc, seq)
    for key in first:
        assert _same(first[key], second[key]) and _same(first[key], third[key]), key
    assert np.array_equal(f1, np.stack(_flags(acc, bound)))
    assert sorted(rec[1].data_ptr() for rec in acc._ledger.values()) == entries, "the entries of the first sweep are reused"
    del second
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) <= before, "a sweep after the first keeps nothing it allocated"
    _assert_same_results(third, _sweep(ops.CalibAccumulators(len(elems), dev, 2048), [(plan, row) for row in xs]))
    _assert_oracle(third["hist"], batches, 2048, _batch_dmax(batches).max(0), (1, 3, 4, 5, 7, 9))


def test_a_dropped_bound_set_is_released(dev):
    ops, spec, batches, elems, plan, acc = _case(dev, 2048, seed=13)
    xs = _upload(batches[:2], dev)
    set_bytes = 4 * B * sum(elems)
    bound = [plan.bind(row) for row in xs]
    del xs
    acc.reset_minmax()
    for i in range(len(bound)):          # (no loop variable left holding a set)
        acc.minmax_accumulate(plan, bound[i])
    torch.cuda.synchronize()
    assert len(acc._ledger) == 2
    before = torch.cuda.memory_allocated(dev)
    dropped = bound.pop()
    del dropped
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) <= before - set_bytes, "the ledger kept a dropped bound set alive"
    assert len(acc._ledger) == 1 and len(acc._slab) == 1, "the dropped set's entry goes back to the slab"
    gmin, gmax = acc.finalize_minmax()
    acc.hist_prepare()
    acc.abs_hist_accumulate(plan, bound[0])
    assert int(acc.hist.sum()) == B * sum(elems)


def test_speculate_false_and_the_refusal_above_the_memory_limit(dev):
    """speculate=False never takes the fused path; a plan whose entry (T * bins * 4 B) would exceed 1/64 of its batch's bytes does
    not either.  Both give the plain path's results."""
    ops, spec, batches, elems, plan, acc = _case(dev, 2048, seed=15, speculate=False)
    xs = _upload(batches, dev)
    bound = [plan.bind(row) for row in xs]
    assert not acc.will_speculate(plan, bound[0])
    got = _sweep(acc, [(plan, x) for x in bound])
    assert acc.spec_flags(bound[0]) is None and acc.spec_stats()["pairs"] == 0 and not acc._ledger
    on = ops.CalibAccumulators(len(elems), dev, 2048)
    assert on.will_speculate(plan, bound[0])
    _assert_same_results(got, _sweep(on, [(plan, x) for x in bound]))
    assert on.spec_stats()["pairs_skipped"] > 0
    fin = _batch_dmax(batches).max(0)
    _assert_oracle(got["hist"], batches, 2048, fin, (1, 2, 5, 6, 7))
    # the limit: T * bins * 4 * 64 <= batch bytes.  16384 bins over this set: 10 * 16384 * 4 * 64 = 42 MB > its 4.6 MB
    wide = ops.CalibAccumulators(len(elems), dev, 16384)
    assert len(elems) * 16384 * 4 * wide.SPEC_MAX_SHARE > plan.total * 4
    assert not wide.will_speculate(plan, bound[0])
    got = _sweep(wide, [(plan, x) for x in bound])
    assert wide.spec_flags(bound[0]) is None and wide.spec_stats()["pairs"] == 0 and not wide._ledger
    _assert_same_results(got, _sweep(ops.CalibAccumulators(len(elems), dev, 16384), [(plan, row) for row in xs]))
    _assert_oracle(got["hist"], batches, 16384, fin, (1, 3, 4, 7, 9))
    # just inside and just outside the limit
    small = ops.TensorSetPlan([1024], 4, dev)          # one tensor of 4096 elements = 64 * bins elements at bins = 64
    a64, a65 = ops.CalibAccumulators(1, dev, 64), ops.CalibAccumulators(1, dev, 65)
    b = small.bind([torch.randn(4, small.elems[0], device=dev)])
    assert a64.will_speculate(small, b) and not a65.will_speculate(small, b)


def test_baseline_size_pool_of_three(dev):
    """bench.py's own sequence at BASELINE size — all 123 ResNet-50 tensors, 32 images per batch, 32 batches — over a pool of
    three bound sets, against the same sequence on plain lists.  (With a pool of three every set but the first visits comes
    behind all extremes: nearly everything is skipped — the benchmark's default pool shows the same artefact.)"""
    from dipoorlet_amd import ops
    from dipoorlet_amd.synthetic import resnet50_tensors, synth_activations
    spec = resnet50_tensors()
    elems = [e for _, e, _ in spec]
    Bn, n_batches = 32, 32
    plan = ops.TensorSetPlan(elems, Bn, dev)
    raw = [synth_activations(spec, Bn, dev, seed=1234 + j) for j in range(3)]
    pool = [plan.bind(x) for x in raw]
    acc = ops.CalibAccumulators(len(elems), dev, 2048)
    assert acc.will_speculate(plan, pool[0])
    got = _sweep(acc, [(plan, pool[b % 3]) for b in range(n_batches)])
    st = acc.spec_stats()
    print("baseline-size pool of 3:", st)
    assert st["pairs"] == n_batches * len(elems)
    # the last visit of every set comes behind every extreme: all of its tensors are valid in all of its histogram-pass visits
    for x in pool:
        assert (acc.spec_flags(x).numpy() == 1).all()
    assert st["pairs_skipped"] == st["pairs"] and st["elements_skipped"] == st["elements"]
    ref = _sweep(ops.CalibAccumulators(len(elems), dev, 2048), [(plan, raw[b % 3]) for b in range(n_batches)])
    _assert_same_results(got, ref)
    assert np.array_equal(got["hist"].sum(1).cpu().numpy(), np.array(elems, np.int64) * Bn * n_batches)
    for t in (0, len(elems) - 1):
        x = np.concatenate([r[t].cpu().numpy().ravel() for r in raw])
        lo, hi = O.minmax(x)
        h = O.abs_hist(x, 2048, O.hist_dmax(lo, hi))
        mult = np.array([11, 11, 10])       # visits of sets 0, 1, 2 in 32 batches
        per_set = [O.abs_hist(r[t].cpu().numpy().ravel(), 2048, O.hist_dmax(lo, hi)) for r in raw]
        assert np.array_equal(sum(per_set), h)
        assert np.array_equal(got["hist"][t].cpu().numpy(), sum(m * p for m, p in zip(mult, per_set)))
