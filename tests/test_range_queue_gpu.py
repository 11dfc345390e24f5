"""GPU: the range pass's schedule (k_minmax_hist: body shares + tail entries claimed from a queue, counters carried across the
entries of one slot; ops.build_range_table) gives what the plain two-read sweep gives, bit for bit.

A whole small sweep — range pass over 3 bound batches, hist_prepare, histogram pass, hist_percentile(0.99999) — runs with
CalibAccumulators(speculate=True) under every shape of the table and is compared for EQUALITY with one speculate=False run of
the same data (computed once per bin count).  Every case also proves that the entry's counts were USED: the skip flags of the
bound sets equal the table the inputs were built for, so a fall-back to the second read cannot pass.

Per-image sizes 1, 7, 1023, 4099, 300 001, 1 500 003 with B = 3: below one aligned piece, odd, unaligned, and large enough that
the big tensors spread over hundreds of blocks (768 body shares of about 6 K elements at the constants as built).
"""
import numpy as np
import pytest

import torch

pytestmark = pytest.mark.gpu

ELEMS = [1, 7, 1023, 4099, 300_001, 1_500_003]
B = 3
K = 3
# what the histogram pass does with tensor t of batch k (1: the range pass's row added, 0: read, 2: nothing to count).  Batch 0 has
# no running range to guess from; tensor 1 is all zeros (the degenerate range, exact path: right from batch 1 on); tensor 2 holds
# a NaN in batch 1 (no range at all); tensors 0, 3 and 5 take their extreme in batch 0, tensor 4 in batch 1.
FLAGS = [[0, 0, 2, 0, 0, 0],
         [1, 1, 2, 1, 0, 1],
         [1, 1, 2, 1, 1, 1]]
PEAK_BATCH = {0: 0, 3: 0, 4: 1, 5: 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    from dipoorlet_amd import _hip
    st, name, _, _ = _hip.device_info()
    assert st == 0, name
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def batches(dev):
    rng = np.random.default_rng(20261)
    out = []
    for k in range(K):
        row = []
        for t, e in enumerate(ELEMS):
            n = B * e
            if t == 1:
                x = np.zeros(n, np.float32)
            else:
                x = np.clip(rng.standard_normal(n).astype(np.float32) * np.float32(0.25), -0.8, 0.8) * np.float32(3.0 + t)
                if t == 5:
                    x = np.maximum(x, 0)        # half zeros: the zero count of carried entries
                if t == 2:
                    if k == 1:
                        x[n // 2] = np.float32("nan")
                elif PEAK_BATCH[t] == k:
                    x[int(rng.integers(0, n))] = np.float32(3.0 + t)
            row.append(torch.from_numpy(x.reshape(B, e)).to(dev))
        out.append(row)
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _sweep(acc, plan, bound):
    acc.reset_minmax()
    for x in bound:
        acc.minmax_accumulate(plan, x)
    acc.finalize_minmax()
    acc.hist_prepare()
    for x in bound:
        acc.abs_hist_accumulate(plan, x)
    clip = acc.hist_percentile(0.99999)
    return {"hist": acc.hist.clone(), "gmin": acc.gmin.clone(), "gmax": acc.gmax.clone(), "clip": clip}


@pytest.fixture(scope="module", params=[2048, 7])
def ref(request, dev, batches):
    """(bins, the two-read sweep's results): speculate=False, computed once and left unchanged."""
    from dipoorlet_amd import ops
    bins = request.param
    plan = ops.TensorSetPlan(ELEMS, B, dev)
    bound = [plan.bind(row) for row in batches]
    acc = ops.CalibAccumulators(len(ELEMS), dev, bins, speculate=False)
    assert not acc.will_speculate(plan, bound[0])
    out = _sweep(acc, plan, bound)
    torch.cuda.synchronize()
    assert int(out["hist"].sum()) > 0
    return bins, out


def _assert_same(got, want):
    for key in ("hist", "gmin", "gmax", "clip"):
        assert got[key].shape == want[key].shape and torch.equal(_bits(got[key]), _bits(want[key])), key


def _assert_flags(acc, bound):
    for k, x in enumerate(bound):
        flags = acc.spec_flags(x)
        assert flags is not None and flags.tolist() == FLAGS[k], (k, flags)     # (rows used, flag 1, in batches 1 and 2)


def _plan(dev, kind=None):
    from dipoorlet_amd import ops
    plan = ops.TensorSetPlan(ELEMS, B, dev)
    if kind is not None:
        plan.range_kind = kind
    return plan


# (the table's shape: None = the constants as built; else ('range', n_body, tail_share, tail_entries)) -> (body blocks, tail entries)
# it must give, so that each case is known to run the path it is there for: the device has 256 CUs, the grid is min(blocks, 768)
SHAPES = {
    "as_built": (None, lambda nb, nt: nb == 768 and 0 < nt),
    "tail_outnumbers_grid": (("range", 8, 0.9, 4000), lambda nb, nt: nb == 8 and nt >= 4 * 768),     # every workgroup claims, several times
    "fewer_blocks_than_grid": (("range", 3, 0.5, 2), lambda nb, nt: nb + nt < 768),                  # nothing to claim from the start
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sweep_equals_two_read_sweep(dev, batches, ref, shape):
    from dipoorlet_amd import ops
    bins, want = ref
    kind, expect = SHAPES[shape]
    plan = _plan(dev, kind)
    bound = [plan.bind(row) for row in batches]
    acc = ops.CalibAccumulators(len(ELEMS), dev, bins, speculate=True)
    assert acc.will_speculate(plan, bound[0])
    w = plan.work(plan.range_kind)
    items, bb, nb, nt = ops.build_range_table(plan._spans(False), *(kind[1:] if kind else (768,)))
    assert expect(nb, nt) and w.n_blocks == nb + nt, (nb, nt)
    got = _sweep(acc, plan, bound)
    _assert_same(got, want)
    _assert_flags(acc, bound)


def test_entry_reused_after_reset(dev, batches, ref):
    """A second sweep over the same entries after reset_minmax(): the queue counter is zeroed with the counts, every launch."""
    from dipoorlet_amd import ops
    bins, want = ref
    plan = _plan(dev, ("range", 8, 0.9, 4000))
    bound = [plan.bind(row) for row in batches]
    acc = ops.CalibAccumulators(len(ELEMS), dev, bins, speculate=True)
    assert acc.will_speculate(plan, bound[0])
    first = _sweep(acc, plan, bound)
    entries = sorted(rec.entry.data_ptr() for rec in acc._ledger.values())
    second = _sweep(acc, plan, bound)
    assert sorted(rec.entry.data_ptr() for rec in acc._ledger.values()) == entries      # the same entries served again
    _assert_same(first, want)
    _assert_same(second, want)
    _assert_flags(acc, bound)


def test_two_accumulators_on_two_streams(dev, batches, ref):
    """Two accumulators driven alternately on two streams over the same bound sets: each entry has its own queue counter."""
    from dipoorlet_amd import ops
    bins, want = ref
    plan = _plan(dev, ("range", 8, 0.9, 4000))
    bound = [plan.bind(row) for row in batches]
    accs = [ops.CalibAccumulators(len(ELEMS), dev, bins, speculate=True) for _ in range(2)]
    assert all(a.will_speculate(plan, bound[0]) for a in accs)
    plan.work(plan.range_kind)      # (the plan's uploads happen here, before the streams part)
    plan.elems_device()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for a, s in zip(accs, streams):
        with torch.cuda.stream(s):
            a.reset_minmax()
    for x in bound:
        for a, s in zip(accs, streams):
            with torch.cuda.stream(s):
                a.minmax_accumulate(plan, x)
    got = []
    for a, s in zip(accs, streams):
        with torch.cuda.stream(s):
            a.finalize_minmax()
            a.hist_prepare()
    for x in bound:
        for a, s in zip(accs, streams):
            with torch.cuda.stream(s):
                a.abs_hist_accumulate(plan, x)
    for a, s in zip(accs, streams):
        with torch.cuda.stream(s):
            clip = a.hist_percentile(0.99999)
        s.synchronize()
        got.append({"hist": a.hist, "gmin": a.gmin, "gmax": a.gmax, "clip": clip})
    torch.cuda.synchronize()
    for a, g in zip(accs, got):
        _assert_same(g, want)
        _assert_flags(a, bound)
