"""CPU: the model of the range pass's histogram speculation (tests/hist_spec_model.py) is held to its properties — the
partition of the remaining element stream covers every remaining element once, never crosses a tensor, cuts on 1024-element
boundaries, gives equal shares and lists nothing of a skipped tensor; the validity table follows the running dmax — and to
the host partition (dpl_build_balanced_items) where nothing is skipped."""
import random

import numpy as np
import pytest

import hist_spec_model as M


def _random_case(rnd):
    T = rnd.randint(1, 40)
    elems = [rnd.choice([0, 1, 3, 1000, 1024, 1025, 4096, 50000, rnd.randint(1, 3_000_000)]) for _ in range(T)]
    skip = [rnd.random() < rnd.choice([0.0, 0.5, 0.9]) for _ in range(T)]
    return elems, skip, rnd.choice([1, 2, 7, 64, 256, 768])


def test_partition_properties():
    rnd = random.Random(11)
    for _ in range(200):
        elems, skip, G = _random_case(rnd)
        blocks = M.partition(elems, skip, G)
        assert len(blocks) == G
        covered = {t: [] for t in range(len(elems))}
        for items in blocks:
            for t, off, cnt in items:
                assert cnt > 0
                assert not skip[t], "a piece of a skipped tensor is listed"
                assert off + cnt <= elems[t], "an item crosses its tensor's end"
                covered[t].append((off, cnt))
        for t, e in enumerate(elems):                   # every remaining element in exactly one item
            pos = 0
            for off, cnt in sorted(covered[t]):
                assert off == pos
                pos += cnt
            assert pos == (0 if skip[t] else e)
        total = sum(e for e, s in zip(elems, skip) if not s)
        sizes = [sum(c for _, _, c in items) for items in blocks]
        assert sum(sizes) == total
        for b, items in enumerate(blocks):              # cuts are 1024-aligned inside a tensor
            for t, off, cnt in items:
                assert off % M.ALIGN == 0, "an item starts off a 1024-element boundary of its tensor"
                assert (off + cnt) % M.ALIGN == 0 or off + cnt == elems[t]
        for s in sizes:                                 # equal shares to within one cut on either side
            assert abs(s - total / G) < M.ALIGN + 1


def test_cuts_are_monotone_and_end_on_the_total():
    rnd = random.Random(5)
    for _ in range(100):
        elems, skip, G = _random_case(rnd)
        c = M.cuts(elems, skip, G)
        assert c[0] == 0 and c[-1] == sum(e for e, s in zip(elems, skip) if not s)
        assert all(a <= b for a, b in zip(c, c[1:]))


def test_partition_equals_the_host_partition_when_nothing_is_skipped():
    from dipoorlet_amd import _hip
    from dipoorlet_amd.csrc import build as hipbuild
    hipbuild.build()
    rnd = random.Random(3)
    for _ in range(40):
        elems, _, G = _random_case(rnd)
        spans = [(t, 0, e, t) for t, e in enumerate(elems)]
        arr, n, bb = _hip.build_balanced_items(spans, G)
        host = [[(arr[i].seg, arr[i].offset, arr[i].count) for i in range(bb[b], bb[b + 1])] for b in range(G)]
        assert host == M.partition(elems, [False] * len(elems), G)


def test_valid_table_follows_the_running_dmax():
    nan = np.nan
    #              t0: extreme first   t1: last   t2: middle   t3: tie (1, 3)   t4: all zero   t5: NaN in batch 2
    d = np.array([[9.0,               1.0,       1.0,         1.0,             0.0,           1.0],
                  [1.0,               2.0,       2.0,         7.0,             0.0,           2.0],
                  [2.0,               3.0,       8.0,         3.0,             0.0,           nan],
                  [3.0,               4.0,       1.0,         7.0,             0.0,           9.0],
                  [4.0,               5.0,       2.0,         2.0,             0.0,           1.0]], np.float32)
    fin = np.array([9.0, 5.0, 8.0, 7.0, 0.0, nan], np.float32)
    v = M.valid_table(d, fin)
    assert not v[0].any(), "the first batch has no running range: no guess"
    assert v[:, 0].tolist() == [False, True, True, True, True]
    assert v[:, 1].tolist() == [False] * 5
    assert v[:, 2].tolist() == [False, False, False, True, True]
    assert v[:, 3].tolist() == [False, False, True, True, True]
    assert v[:, 4].tolist() == [False, True, True, True, True]
    assert v[:, 5].tolist() == [False] * 5
    # a merged range larger than this shard's: nothing is valid; the sign of a zero counts (the comparison is on bits)
    assert not M.valid_table(d, fin * 2)[:, :4].any()
    assert not M.valid_table(d, np.array([9.0, 5.0, 8.0, 7.0, -0.0, nan], np.float32))[:, 4].any()
    # range_ok = False (numpy refuses the range): never valid
    assert not M.valid_table(d, fin, range_ok=[False] * 6).any()
    assert M.skipped_share(v, [1, 1, 1, 1, 1, 1]) == pytest.approx((4 + 0 + 2 + 3 + 4 + 0) / 30)


def test_exchangeable_batches_skip_about_half():
    """The reasoning behind the change: with n exchangeable batches the batch holding a tensor's extreme is uniform over the n,
    so the pairs behind it — (n - 1) / 2 of n on average — need no second read."""
    rng = np.random.default_rng(0)
    K, T = 32, 123
    shares = []
    for _ in range(200):
        d = rng.random((K, T)).astype(np.float32)
        shares.append(M.skipped_share(M.valid_table(d, d.max(0)), np.ones(T)))
    assert np.mean(shares) == pytest.approx((K - 1) / (2 * K), abs=0.01)
