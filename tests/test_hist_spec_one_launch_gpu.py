"""GPU: the histogram pass over a bound set as ONE launch (k_hist_spec, csrc/calib_kernels.hip K2s) at the smallest shapes at which
it can go wrong: more slots than workgroups (the resolver loop), fewer slots than workgroups with uneven tensors (cuts inside a
tensor, at a tensor boundary and in a scalar tail), nothing left to read, nothing valid, an entry consumed several times, the four
statistics words, ranges merged between the passes.

The expected flags and cuts come from the model (tests/hist_spec_model.py), the expected histograms and clips from the plain path
(CalibAccumulators(..., speculate=False)): every comparison is for equality.  Every test first asserts that the set speculates,
so none can pass on the plain path alone.
"""
import ctypes as C

import numpy as np
import pytest

import torch

import hist_spec_model as M
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

B = 2                                       # images per batch
UNEVEN = [1, 1023, 1025, 4099, 70001]       # per image: below, around and above the 1024-element alignment of a cut
UNEVEN_PEAKS = [0, 2, 1, 3, 1]              # the batch that holds each tensor's extreme (of 4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    from dipoorlet_amd import _hip
    st, name, _, _ = _hip.device_info()
    assert st == 0, name
    return torch.device("cuda:0")


def _make(elems, peaks, n_batches, seed):
    """-> batches[k][t]: float32 numpy [B, elems[t]].  |values| <= 0.8 * peak_t except the planted extreme (+peak_t, or -peak_t
    for odd t: dmax from the minimum) in batch peaks[t]; every third tensor is a ReLU output (about half exact zeros)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_batches):
        row = []
        for t, e in enumerate(elems):
            peak = np.float32(1.0 + 0.125 * (t % 11))
            x = (rng.uniform(-0.8, 0.8, B * e).astype(np.float32) * peak).astype(np.float32)
            if t % 3 == 0:
                x = np.maximum(x, np.float32(0))
            if k == peaks[t]:
                x[int(rng.integers(0, B * e))] = -peak if t % 2 else peak
            row.append(x.reshape(B, e))
        out.append(row)
    return out


def _batch_dmax(batches):
    d = np.zeros((len(batches), len(batches[0])), np.float32)
    for k, row in enumerate(batches):
        for t, x in enumerate(row):
            d[k, t] = O.hist_dmax(*O.minmax(x))
    return d


def _final_dmax(dmax):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(dmax).any(0), np.float32(np.nan), dmax.max(0)).astype(np.float32)


def _range_ok(fin, bins):
    ok = []
    for d in fin:
        try:
            np.histogram(np.zeros(1, np.float32), bins, (0, np.float32(d)))
            ok.append(True)
        except ValueError:
            ok.append(False)
    return np.array(ok)


def _sweep(acc, p1, p2=None, merged=None):
    """bench.py's sequence: p1 = the (plan, tensors) of the range pass, p2 of the histogram pass (default: the same)."""
    acc.reset_minmax()
    for plan, x in p1:
        acc.minmax_accumulate(plan, x)
    gmin, gmax = acc.finalize_minmax()
    if merged is not None:
        acc.set_minmax(*merged(gmin.clone(), gmax.clone()))
    acc.hist_prepare()
    for plan, x in (p1 if p2 is None else p2):
        acc.abs_hist_accumulate(plan, x)
    return {"hist": acc.hist.clone(), "clip": acc.hist_percentile(0.99999)}


def _assert_equal(got, ref):
    assert torch.equal(got["hist"], ref["hist"]), "hist differs from the plain path"
    assert torch.equal(got["clip"].view(torch.int32), ref["clip"].view(torch.int32)), "clip differs from the plain path"


def _setup(dev, elems, peaks, n_batches, bins, seed, share=None):
    """-> ops, plan, batches, bound sets, the speculating accumulator, the plain one.  `share`: the accumulator's SPEC_MAX_SHARE
    (a limit on an entry's size against its batch, which says when speculation pays, not when it is right)."""
    from dipoorlet_amd import ops
    batches = _make(elems, peaks, n_batches, seed)
    plan = ops.TensorSetPlan(elems, B, dev)
    acc = ops.CalibAccumulators(len(elems), dev, bins)
    if share is not None:
        acc.SPEC_MAX_SHARE = share
    assert len(elems) * bins * acc.SPEC_MAX_SHARE <= plan.total, "the set must be large enough for its entry (SPEC_MAX_SHARE)"
    bound = [plan.bind([torch.from_numpy(x).to(dev) for x in row]) for row in batches]
    assert all(acc.will_speculate(plan, x) for x in bound)
    plain = ops.CalibAccumulators(len(elems), dev, bins, speculate=False)
    assert not plain.will_speculate(plan, bound[0])
    return ops, plan, batches, bound, acc, plain


def _model(batches, bins):
    dmax = _batch_dmax(batches)
    fin = _final_dmax(dmax)
    ok = _range_ok(np.nan_to_num(fin), bins) & ~np.isnan(fin)
    return M.valid_table(dmax, fin, ok), ok


def _expect_stats(valid_rows, e_batch):
    """The model's statistics over the histogram-pass calls whose rows of the table are `valid_rows` [calls, T]."""
    v = np.asarray(valid_rows, bool)
    return {"pairs": int(v.size), "pairs_skipped": int(v.sum()), "elements": int(v.shape[0] * e_batch.sum()),
            "elements_skipped": int((v * e_batch[None, :]).sum())}


def _assert_flags_and_cuts(acc, plan, bound, valid, ok, e_batch):
    nb = plan.work("hist").n_blocks
    for k, x in enumerate(bound):
        flags = acc.spec_flags(x).numpy()
        assert np.array_equal(flags == 1, valid[k]), "batch %d: the skip flags differ from the model's table" % k
        assert np.array_equal(flags == 2, ~ok), "batch %d: flag 2 marks exactly the slots numpy refuses" % k
        assert acc.spec_cuts(plan, x).numpy().tolist() == M.cuts(e_batch.tolist(), (flags != 0).tolist(), nb), k


def test_more_slots_than_workgroups(dev):
    """T = 300 tensors of 64 .. 257 elements per image, 4 bins: the "hist" work set has 24 workgroups, so every workgroup resolves
    twelve or thirteen slots (t = b, b + G, ...).  Extremes in batch t mod 4: every batch has added, read and mixed workgroups."""
    T, bins, n_batches = 300, 4, 4
    elems = [64 + (t * 37) % 194 for t in range(T)]
    assert min(elems) == 64 and max(elems) == 257
    ops, plan, batches, bound, acc, plain = _setup(dev, elems, [t % n_batches for t in range(T)], n_batches, bins, seed=1)
    assert plan.work("hist").n_blocks < T
    valid, ok = _model(batches, bins)
    assert ok.all() and [int(valid[:, t].sum()) for t in range(4)] == [3, 2, 1, 0]
    got = _sweep(acc, [(plan, x) for x in bound])
    e_batch = np.array(elems, np.int64) * B
    _assert_flags_and_cuts(acc, plan, bound, valid, ok, e_batch)
    assert acc.spec_stats() == _expect_stats(valid, e_batch)
    _assert_equal(got, _sweep(plain, [(plan, x) for x in bound]))
    assert np.array_equal(got["hist"].sum(1).cpu().numpy(), e_batch * n_batches)


@pytest.mark.parametrize("bins", [16, 2048])
def test_fewer_slots_than_workgroups_uneven_tensors(dev, bins):
    """Per-image counts 1, 1023, 1025, 4099, 70001 over 38 workgroups: the remaining stream's cuts fall inside the large tensor,
    on tensor boundaries (tensors shorter than the 1024-element alignment) and leave scalar tails (counts that are no multiple of
    four).  At 2048 bins the five rows are 1/4 of the batch, above the accumulator's default share of 1/64: the share is lowered
    on this accumulator (a performance limit: the kernel is the same)."""
    ops, plan, batches, bound, acc, plain = _setup(dev, UNEVEN, UNEVEN_PEAKS, 4, bins, seed=2, share=64 if bins == 16 else 8)
    assert plan.work("hist").n_blocks > len(UNEVEN)
    valid, ok = _model(batches, bins)
    assert ok.all() and valid.sum(0).tolist() == [3, 1, 2, 0, 2]
    got = _sweep(acc, [(plan, x) for x in bound])
    e_batch = np.array(UNEVEN, np.int64) * B
    _assert_flags_and_cuts(acc, plan, bound, valid, ok, e_batch)
    # (what the cases are chosen for, read off the model's cuts, which the device's were just held to)
    inside = boundary = empty = False
    for k in range(len(bound)):
        rem = [0 if s else int(e) for e, s in zip(e_batch, valid[k])]
        P = np.concatenate([[0], np.cumsum(rem)])
        c = np.array(M.cuts(e_batch.tolist(), valid[k].tolist(), plan.work("hist").n_blocks))
        starts = {int(P[t]) for t in range(len(rem)) if rem[t] and P[t] > 0}
        inside |= any(int(x) not in set(P.tolist()) for x in c)
        boundary |= any(int(x) in starts for x in c)
        empty |= bool(((np.diff(c) == 0) & (c[:-1] < P[-1])).any())
    assert inside and boundary and empty, "a cut inside a tensor, one on a tensor boundary, a workgroup with no share"
    assert acc.spec_stats() == _expect_stats(valid, e_batch)
    _assert_equal(got, _sweep(plain, [(plan, x) for x in bound]))
    for t in range(len(UNEVEN)):
        x = np.concatenate([row[t].ravel() for row in batches])
        assert np.array_equal(got["hist"][t].cpu().numpy(), O.abs_hist(x, bins, _batch_dmax(batches).max(0)[t])), t


def test_nothing_left_to_read(dev):
    """The range pass sees the set twice, so its second visit guesses every range right: every flag is 1, every cut is zero (each
    workgroup returns after its resolver duty) and hist is the entry's rows."""
    bins = 16
    ops, plan, batches, bound, acc, plain = _setup(dev, UNEVEN, [0] * 5, 1, bins, seed=3)
    A = bound[0]
    got = _sweep(acc, [(plan, A), (plan, A)], [(plan, A)])
    assert (acc.spec_flags(A).numpy() == 1).all()
    cuts = acc.spec_cuts(plan, A).numpy()
    assert cuts.shape == (plan.work("hist").n_blocks + 1,) and not cuts.any()
    e_batch = np.array(UNEVEN, np.int64) * B
    assert acc.spec_stats() == _expect_stats(np.ones((1, 5), bool), e_batch)
    _assert_equal(got, _sweep(plain, [(plan, A), (plan, A)], [(plan, A)]))
    assert np.array_equal(got["hist"].sum(1).cpu().numpy(), e_batch)


def test_nothing_valid(dev):
    """The first batch of a sweep has no guess (snapshot status != 0): everything is read.  A NaN in one tensor makes its final
    range's status != 0: flag 2 for that slot in every batch, nothing of it counted, every other slot as the model says."""
    bins = 16
    ops, plan, batches, bound, acc, plain = _setup(dev, UNEVEN, UNEVEN_PEAKS, 4, bins, seed=4)
    e_batch = np.array(UNEVEN, np.int64) * B
    got = _sweep(acc, [(plan, bound[0])])
    assert not acc.spec_flags(bound[0]).numpy().any()
    assert acc.spec_stats(reset=True) == _expect_stats(np.zeros((1, 5), bool), e_batch)
    _assert_equal(got, _sweep(plain, [(plan, bound[0])]))
    assert np.array_equal(got["hist"].sum(1).cpu().numpy(), e_batch)
    # ... a NaN in tensor 2 of batch 1
    batches[1][2][1, 7] = np.nan
    bound[1] = plan.bind([torch.from_numpy(x).to(dev) for x in batches[1]])
    assert acc.will_speculate(plan, bound[1])
    valid, ok = _model(batches, bins)
    assert ok.tolist() == [True, True, False, True, True] and valid.sum(0).tolist() == [3, 1, 0, 0, 2]
    got = _sweep(acc, [(plan, x) for x in bound])
    _assert_flags_and_cuts(acc, plan, bound, valid, ok, e_batch)
    assert acc.spec_stats() == _expect_stats(valid, e_batch)
    assert acc.range_status()["status"][2] == 1 and int(got["hist"][2].sum()) == 0
    _assert_equal(got, _sweep(plain, [(plan, x) for x in bound]))


def test_one_entry_consumed_three_times(dev):
    """Three histogram passes over the same bound set add its valid rows three times and read the rest three times: the entry's
    snapshot and counts are only read."""
    bins = 16
    ops, plan, batches, bound, acc, plain = _setup(dev, UNEVEN, UNEVEN_PEAKS, 4, bins, seed=5)
    valid, ok = _model(batches, bins)
    assert 0 < valid[2].sum() < len(UNEVEN), "the set consumed three times has rows to add and tensors to read"
    p1 = [(plan, x) for x in bound]
    p2 = [(plan, bound[2])] * 3
    got = _sweep(acc, p1, p2)
    e_batch = np.array(UNEVEN, np.int64) * B
    assert np.array_equal(acc.spec_flags(bound[2]).numpy() == 1, valid[2])
    assert acc.spec_stats() == _expect_stats(np.stack([valid[2]] * 3), e_batch)
    _assert_equal(got, _sweep(plain, p1, p2))
    assert np.array_equal(got["hist"].sum(1).cpu().numpy(), 3 * e_batch)
    single = _sweep(acc, p1, p2[:1])
    assert torch.equal(got["hist"], 3 * single["hist"])


def test_stats_are_exact_and_may_be_null(dev):
    """spec_stats() after a mixed sweep equals the model's four numbers.  CalibAccumulators always passes its statistics words, so
    the null form (the C ABI allows d_stats == NULL) is reached by calling dpl_hist_spec_accumulate itself on the accumulator's
    entry: the words stay what they were, the flags and the histogram are those of one more pass over the batch."""
    from dipoorlet_amd import _hip
    bins = 16
    ops, plan, batches, bound, acc, plain = _setup(dev, UNEVEN, UNEVEN_PEAKS, 4, bins, seed=6)
    valid, ok = _model(batches, bins)
    e_batch = np.array(UNEVEN, np.int64) * B
    p1 = [(plan, x) for x in bound]
    _sweep(acc, p1)
    expect = _expect_stats(valid, e_batch)
    assert 0 < expect["pairs_skipped"] < expect["pairs"] and 0 < expect["elements_skipped"] < expect["elements"]
    assert acc.spec_stats() == expect
    x = bound[1]
    entry = acc._entry_of(plan, x)
    assert entry is not None
    _hip.check(_hip.lib().dpl_hist_spec_accumulate(ops._ptr(entry), ops._ptr(plan.elems_device()), plan.T, plan.work("hist").n_blocks,
                                                   ops._ptr(plan.seg_table(x)), ops._ptr(acc.ranges), bins, ops._ptr(acc.hist),
                                                   C.c_void_p(None), ops._stream()), "dpl_hist_spec_accumulate")
    assert acc.spec_stats() == expect, "a null d_stats leaves the statistics alone"
    assert np.array_equal(acc.spec_flags(x).numpy() == 1, valid[1])
    ref = _sweep(plain, p1, p1 + [(plan, x)])
    assert torch.equal(acc.hist, ref["hist"])


def test_merged_ranges_on_some_slots(dev):
    """set_minmax between the passes with a larger range on slots 1 and 4: those are read in every batch (their guesses cannot
    equal the merged range), the others are added as the model says."""
    bins = 16
    ops, plan, batches, bound, acc, plain = _setup(dev, UNEVEN, UNEVEN_PEAKS, 4, bins, seed=7)
    valid, ok = _model(batches, bins)
    sel = torch.tensor([False, True, False, False, True], device=dev)

    def merged(lo, hi):
        return torch.where(sel, lo * 2 - 1, lo), torch.where(sel, hi * 2 + 1, hi)
    expect = valid & ~sel.cpu().numpy()[None, :]
    assert expect.any() and (valid & ~expect).any(), "the merge must take guesses away and leave some"
    p1 = [(plan, x) for x in bound]
    got = _sweep(acc, p1, merged=merged)
    e_batch = np.array(UNEVEN, np.int64) * B
    _assert_flags_and_cuts(acc, plan, bound, expect, ok, e_batch)
    assert acc.spec_stats() == _expect_stats(expect, e_batch)
    _assert_equal(got, _sweep(plain, p1, merged=merged))
