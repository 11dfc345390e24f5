"""The two-part work table of the range pass (ops.build_range_table, work kind 'range'): body shares + queue-claimed tail entries
cover the element stream exactly once, tail entries never cross a tensor, and a ledger entry has room for the queue counter
behind its counts.  Host only: the builder is dpl_build_balanced_items."""
import ctypes as C

import numpy as np
import pytest

from dipoorlet_amd import _hip, ops
from dipoorlet_amd.synthetic import resnet50_tensors

SMALL = [1, 7, 1023, 4099, 300_001, 1_500_003]


def _spans(elems, batch):
    return [(t, 0, e * batch, t) for t, e in enumerate(elems)]


def _blocks(items, bb):
    return [items[bb[b]:bb[b + 1]] for b in range(len(bb) - 1)]


@pytest.mark.parametrize("elems,batch,n_body,share,n_entries", [
    (SMALL, 3, 768, ops.RANGE_TAIL_SHARE, ops.RANGE_TAIL_ENTRIES),          # the plan as built at the GPU test's shapes
    (SMALL, 3, 8, 0.9, 4000),                                               # tail entries outnumber any grid many times
    (SMALL, 3, 3, 0.5, 2),                                                  # fewer entries than workgroups
    (SMALL, 3, 768, 0.0, 0),                                                # no tail at all
    ([5], 1, 768, ops.RANGE_TAIL_SHARE, ops.RANGE_TAIL_ENTRIES),            # a stream shorter than one aligned piece
    ([e for _, e, _ in resnet50_tensors()], 32, 768, ops.RANGE_TAIL_SHARE, ops.RANGE_TAIL_ENTRIES),     # the flagship batch
])
def test_table_covers_the_stream_once(elems, batch, n_body, share, n_entries):
    spans = _spans(elems, batch)
    items, bb, nb, nt = ops.build_range_table(spans, n_body, share, n_entries)
    assert bb.dtype == np.uint32 and len(bb) == nb + nt + 1 and bb[0] == 0 and bb[-1] == len(items)
    assert np.all(np.diff(bb.astype(np.int64)) >= 0)
    assert nb <= n_body
    # every tensor's pieces, sorted by offset, tile [0, count) with no gap and no overlap
    for seg, off, cnt, slot in spans:
        mine = items[items["seg"] == seg]
        assert np.all(mine["slot"] == slot)
        mine = mine[np.argsort(mine["offset"], kind="stable")]
        assert np.all(mine["count"] > 0)
        starts, ends = mine["offset"].astype(np.int64), mine["offset"].astype(np.int64) + mine["count"]
        assert starts[0] == off and ends[-1] == off + cnt and np.array_equal(starts[1:], ends[:-1])
        assert np.all((starts[1:] - off) % 1024 == 0)       # cuts inside a tensor stay 4 KiB-aligned
    assert int(items["count"].astype(np.int64).sum()) == sum(e * batch for e in elems)
    # a tail entry is one item: it cannot cross a tensor
    blocks = _blocks(items, bb)
    assert all(len(b) == 1 for b in blocks[nb:])
    # the body comes first in the stream, the tail behind it; the tail's share is what was asked for (to one entry's rounding)
    tail_total = int(sum(int(b["count"][0]) for b in blocks[nb:]))
    total = sum(e * batch for e in elems)
    if n_entries == 0:
        assert nt == 0
    elif total >= 1 << 20:
        assert abs(tail_total - total * share) <= max(1024, total // max(nb, 1))
        assert 0.5 * n_entries <= nt <= 2 * n_entries or min(elems) * batch < 1024 * 4


def test_tail_is_round_major():
    """The tail's entries lie in n_body contiguous runs of the stream, the table holds the runs' first entries, then their second
    ones, ...: the successive claims of one workgroup, n_body places apart, are neighbours in the stream."""
    elems = [e for _, e, _ in resnet50_tensors()]
    items, bb, nb, nt = ops.build_range_table(_spans(elems, 32), 768)
    assert nb == 768 and nt >= 2 * nb
    tail = items[bb[nb]:]
    key = tail["seg"].astype(np.int64) * (1 << 40) + tail["offset"].astype(np.int64)    # position in the stream
    rank = np.argsort(np.argsort(key))
    assert np.all(np.diff(rank[:nb]) > 0)                           # round 0: one entry of every run, in stream order
    assert np.array_equal(rank[nb:2 * nb], rank[:nb] + 1)           # round 1: each run's next entry
    same_slot_next = np.mean(tail["slot"][:nt - nb] == tail["slot"][nb:])
    assert same_slot_next > 0.9, same_slot_next     # a workgroup's next claim is almost always in the tensor it is on


def test_entry_has_room_for_the_queue():
    L = _hip.lib()
    for n_slots, bins in [(1, 1), (6, 7), (6, 2048), (53, 2048), (557, 16384)]:
        nbytes = int(L.dpl_hist_spec_entry_bytes(n_slots, bins))
        counts_off = (n_slots * (C.sizeof(_hip.HistRange) + 4) + 15) & ~15
        assert nbytes % 16 == 0
        assert nbytes >= counts_off + n_slots * bins * 4 + 16      # 16 bytes behind the counts' end
