"""What the HOST planning of the C ABI (csrc/host_plan.hpp) must satisfy, whoever computed it — the shipped library through
ctypes (test_capi_load.py) or the stand-alone sanitizer build (test_host_plan_host.py) — and the span sets both are given.
Items are tuples (seg, offset, count, slot[, reserved]); spans are (seg, offset, count, slot)."""
import random


def balanced_sets():
    """The random span sets of test_build_balanced_items_host: (spans, n_blocks)."""
    rnd = random.Random(4)
    for _ in range(30):
        spans = [(i, rnd.choice([0, 16, 4096]), rnd.choice([0, 1, 1000, 2048, 25088, 401408, 802816 * 16]), 100 + i)
                 for i in range(rnd.randint(1, 12))]
        yield spans, rnd.choice([1, 2, 7, 64, 512])


def slice_sets(cap):
    """The random span sets of test_build_octav_slices_host (slots 0 .. n-1 in order: a plan takes them too)."""
    rnd = random.Random(9)
    for _ in range(20):
        n = rnd.randint(1, 40)
        yield [(i % 5, 1000 * i, rnd.choice([0, 1, 3, 777, 20480, 20481, 401408, cap, cap + 1, 802816, 3 * cap + 5]), i)
               for i in range(n)]


def check_cover(spans, items):
    """Every element of every span exactly once and in order, segments and slots preserved, no empty item (spans carry distinct
    slots)."""
    by_slot = {}
    for it in items:
        by_slot.setdefault(it[3], []).append(it)
    assert len({sp[3] for sp in spans}) == len(spans)
    assert set(by_slot) <= {sp[3] for sp in spans}
    for seg, off, cnt, slot in spans:
        pos = off
        for it in by_slot.get(slot, []):
            assert it[0] == seg and it[1] == pos and it[2] > 0, (it, seg, pos)
            pos += it[2]
        assert pos == off + cnt


def check_work_items(spans, chunk, items):
    check_cover(spans, items)
    start = {sp[3]: sp[1] for sp in spans}
    for it in items:
        assert it[2] <= chunk and (it[1] - start[it[3]]) % chunk == 0


def check_balanced(spans, nb, items, bb):
    n = len(items)
    assert len(bb) == nb + 1 and bb[0] == 0 and bb[nb] == n and all(bb[i] <= bb[i + 1] for i in range(nb))
    check_cover(spans, items)
    # shares are balanced to within one aligned piece per span boundary
    total = sum(c for _, _, c, _ in spans)
    share = [sum(items[k][2] for k in range(bb[b], bb[b + 1])) for b in range(nb)]
    assert sum(share) == total
    if total >= nb * 8192:
        assert max(share) <= total / nb + 1024 * (len(spans) + 1)
    # cuts inside a span are 4 KiB aligned relative to the span start
    start = {sp[3]: sp[1] for sp in spans}
    for it in items:
        assert (it[1] - start[it[3]]) % 1024 == 0


def check_slices(spans, cap, items, ps):
    """Every pair cut into ceil(count / cap) equal slices on multiples of 4 elements, largest pairs first, pair_slice0 = the
    pair's contiguous slice range (spans carry slots 0 .. n-1)."""
    sizes_seen = []
    for seg, off, cnt, slot in spans:
        lo, hi = ps[2 * slot], ps[2 * slot + 1]
        want = 0 if cnt == 0 else -(-cnt // cap)
        assert hi - lo == want
        pos = off
        for k in range(lo, hi):
            s_, o, c, sl, res = items[k]
            assert (s_, o, sl, res) == (seg, pos, slot, want) and 0 < c <= cap
            assert (o - off) % 4 == 0
            if k + 1 < hi:
                assert c % 4 == 0 and c == items[lo][2]          # equal slices; only the last one takes the remainder
            pos += c
        assert pos == off + cnt
        if want:
            sizes_seen.append((lo, cnt))
    assert sum(-(-c // cap) for _, c in sizes_seen) == len(items)
    order = [c for _, c in sorted(sizes_seen)]
    assert order == sorted(order, reverse=True)                   # largest pairs first


def list_regions(elems, cap, list_cap):
    """(pair_base, pair_base_full) of pairs of `elems` elements: a single-slice pair dpl_octav_list_cap(n) values, a pair of c
    slices c parts of dpl_octav_list_cap(slice); whole-pair regions rounded up to 32 values."""
    base, full = [0], [0]
    for n in elems:
        c = -(-n // cap)
        per = 0 if c == 0 else (-(-n // c) + 3) & ~3
        base.append(base[-1] + (list_cap(n) if c == 1 else c * list_cap(per)))
        full.append(full[-1] + (n + 31) // 32 * 32)
    return base, full


def check_plan_sizes(z, elems, n_tensors, cap, list_cap):
    """dpl_octav_workspace_sizes `z` of a plan over pairs of `elems` elements: sizes follow from the spans alone."""
    P = len(elems)
    base, full = list_regions(elems, cap, list_cap)
    multi = [-(-n // cap) for n in elems if n > cap]
    assert z.list_bytes == 4 * max(base[-1], 32)
    assert z.fallback_bytes == 2 * 4 * max(full[-1], 32)
    assert (z.n_pairs, z.n_slices, z.n_multi, z.n_small) == (P, sum(-(-n // cap) for n in elems), len(multi), sum(n <= 20480 for n in elems))
    assert z.history_bytes == 4 * 2 * n_tensors * 64 and z.result_bytes == 4 * 3 * P
    low = 8 * 2048 * sum(multi) + 8 * 3072 * P
    assert low <= z.rescue_bytes < low + 4096 + 4 * 67 * P
    assert z.state_bytes >= 80 * (P + 1) + 4 * 128 * n_tensors and z.tables_bytes % 256 == 0


TABLE_FIELDS = ("d_slices", "d_pair_slice0", "d_pair_spans", "d_pair_base", "d_pair_base_full", "d_pair_order", "d_items", "d_block_begin")


def check_job(job, z, addr, call_index, dynamic_sym, max_iters):
    """A job bound to the addresses `addr` = (tables, history, state, rescue, list0, list1, fallback or None, seg_ptrs): the
    tables' pointers fall inside the tables block, the lists where they were put, the epoch fields follow the call index."""
    tables, history, state, rescue, list0, list1, fallback, seg_ptrs = addr
    for f in TABLE_FIELDS:
        assert tables <= getattr(job, f) < tables + z.tables_bytes and getattr(job, f) % 256 == 0, f
    assert job.d_vis == history and job.d_states == state and job.d_rescue_bm == rescue
    assert state < job.d_pred < state + z.state_bytes
    assert rescue < job.d_missed < job.d_resc < job.d_lh <= rescue + z.rescue_bytes
    assert job.d_list0 == list0 and job.d_list1 == list1 and job.d_seg_ptrs == seg_ptrs
    if fallback is None:
        assert job.compaction_inline == 0 and job.d_clist0 is None and job.d_clist1 is None
    else:
        assert job.compaction_inline == 1 and job.d_clist0 == fallback and job.d_clist1 - job.d_clist0 == z.fallback_bytes // 2
    assert (job.write_epoch, job.reset_epoch) == (call_index // 8 % 2, int(call_index % 8 == 0))
    assert (job.dynamic_sym, job.max_iters) == (dynamic_sym, max_iters)
    assert (job.n_pairs, job.n_slices, job.n_multi, job.n_small) == (z.n_pairs, z.n_slices, z.n_multi, z.n_small)


SIX_STATES = [(2, 1, 1000), (1, 0, 1000), (3, 0, 50), (1, 1, 77), (1, 0, 33), (0, 0, 9)]   # (mode, done, n_elems)


def fallback_layout(states):
    """dpl_octav_fallback_layout in python: states = (mode, done, n_elems) -> base [n + 1]."""
    base = [0]
    for mode, done, n in states:
        base.append(base[-1] + ((n + 31) // 32 * 32 if mode == 1 and not done else 0))
    return base
