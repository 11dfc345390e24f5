"""CPU: the definition of `-A kl` (tests/kl_model.py) — its two statements agree, it clips where one expects on seeded
tensors, and the host layers know the new key without the reference-mirroring registry having changed."""
import numpy as np
import pytest

import kl_model as M


def _small_histograms():
    """(name, h, L): small enough for the loop-per-bin statement — the fixtures' shapes at 128 and 200 bins, and sparse
    low-count histograms that reach the corners (empty groups, a last bin alive through the outliers alone, candidates that
    are not admissible)."""
    out = []
    for kind in M.KINDS:
        x = M.fixture_tensor(kind)
        for bins, L in ((128, 32), (200, 128), (96, 7)):
            out.append((f"{kind}/{bins}/{L}", M.abs_hist(x, bins)[0], L))
    rng = np.random.default_rng(20)
    for t in range(24):
        bins = int(rng.integers(8, 160))
        L = int(rng.integers(2, min(bins, 40) + 1))
        h = (rng.random(bins) < rng.uniform(0.02, 0.6)) * rng.integers(1, 4, bins)
        out.append((f"sparse{t}/{bins}/{L}", h.astype(np.int64), L))
    out.append(("empty/64/8", np.zeros(64, np.int64), 8))
    return out


def test_two_statements_of_the_model_agree():
    for name, h, L in _small_histograms():
        a, b = M.kl_curve(h, L), M.kl_curve_scalar(h, L)
        assert a.shape == b.shape == (h.size + 1,)
        assert np.all(np.isposinf(a[:L])) and np.all(np.isposinf(b[:L])), name
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), name            # the same admissible set
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        f = np.isfinite(a)
        assert np.allclose(a[f], b[f], rtol=1e-12, atol=1e-15), (name, float(np.abs(a[f] - b[f]).max()))
        assert M.kl_best(a) == M.kl_best(b), name


def test_best_is_the_lowest_minimum_and_nan_never_wins():
    assert M.kl_best(np.array([np.inf, np.nan, 3.0, 1.0, 1.0, 2.0])) == 3
    assert M.kl_best(np.array([np.inf, np.nan, np.inf])) == -1
    assert M.kl_best(np.array([np.nan, -1.0])) == 1


def test_clip_is_the_centre_of_the_last_kept_bin_in_fp32():
    c = M.kl_clip_from_best(1919, np.float32(-4.5), np.float32(4.9), 2048)
    cv = np.float32(np.float32(1918.5) * np.float32(np.float32(4.9) / np.float32(2048)))
    assert c.dtype == np.float32 and c[0] == np.float32(-4.5) and c[1] == cv      # lo: max(-cv, gmin), hi: min(cv, gmax)
    assert np.array_equal(M.kl_clip_from_best(-1, -1.0, 2.0, 128), np.array([-1.0, 2.0], np.float32))


@pytest.fixture(scope="module")
def curves():
    """{(kind, bins): (h, gmin, gmax, clip, best, curve)} at L = 128."""
    out = {}
    for kind in M.KINDS:
        x = M.fixture_tensor(kind)
        for bins in (2048, 1000):
            h, gmin, gmax = M.abs_hist(x, bins)
            out[kind, bins] = (h, gmin, gmax) + M.kl_clip(h, gmin, gmax, 128)
    return out


def test_every_candidate_of_a_non_degenerate_tensor_is_admissible(curves):
    for (kind, bins), (h, _, _, _, best, curve) in curves.items():
        adm = np.isfinite(curve)
        assert not adm[:128].any() and not np.isnan(curve).any()
        if kind == "constant":      # one bin holds everything: only "keep all" leaves q a non-zero bin
            assert adm.sum() == 1 and best == bins and curve[bins] == 0.0
        elif kind == "zeros":       # (the expanded range puts |0| in the middle bin: every cut above it keeps all)
            assert best == bins // 2 + 1 and np.all(curve[adm] == 0.0) and adm.sum() == bins // 2
        elif kind == "two_level":   # two bins: a cut below the upper one folds it into a bin of its own or onto the lower one
            assert adm[bins] and curve[bins] == 0.0 and best == bins
        else:
            assert adm[128:].all(), (kind, bins, int(adm.sum()))


def test_the_search_clips_where_one_expects(curves):
    for bins in (2048, 1000):
        _, gmin, gmax, clip, best, _ = curves["normal", bins]        # 8e5 samples: the range ends near 4.9 sigma
        assert 3.5 < clip[1] <= gmax and clip[0] >= gmin and 128 <= best <= bins
        _, gmin, gmax, clip, best, _ = curves["uniform", bins]       # flat: nothing to gain from clipping
        assert best == bins
        _, gmin, gmax, clip, best, _ = curves["outliers", bins]      # five values at 55 - 78 on a normal body
        assert gmax == 78.0 and 3.0 < clip[1] < 12.0 and clip[0] == -clip[1]
        _, gmin, gmax, clip, best, _ = curves["lognormal", bins]     # heavy tail: far below its maximum
        assert gmax > 150 and clip[1] < 60
        _, gmin, gmax, clip, best, _ = curves["relu", bins]
        assert clip[0] == 0.0 and 0 < clip[1] <= gmax
        for kind in M.KINDS:                                         # always inside the range
            _, gmin, gmax, clip, _, _ = curves[kind, bins]
            assert gmin <= clip[0] <= 0.0 or clip[0] == gmin
            assert clip[1] <= gmax


def test_the_minimum_is_not_a_near_tie(curves):
    """The kernel test allows `best` to differ from i* where the model itself cannot tell two candidates apart (within
    1e-9 relative + 1e-12): on these tensors it can, by an order of magnitude and more (the closest pair, the two lowest
    candidates of the outlier tensor, lies 2e-11 apart at 1.2e-4; fp64 summation noise is 1e-15)."""
    for (kind, bins), (_, _, _, _, best, curve) in curves.items():
        if kind in M.DEGENERATE:
            continue
        others = np.delete(np.where(np.isnan(curve), np.inf, curve), best)
        gap = others.min() - curve[best]
        assert gap > 10 * (1e-9 * abs(curve[best]) + 1e-12), (kind, bins, gap, curve[best])


def test_cli_and_registries_know_kl():
    from dipoorlet_amd.__main__ import build_parser
    from dipoorlet_amd.tensor_cali import find_clip_val_kl, tensor_cali_dispatcher, tensor_cali_extensions
    from dipoorlet_amd.tensor_cali.basic_algorithm import kl_levels
    a = build_parser().parse_args(["-I", "x", "-N", "8", "-D", "trt", "-A", "kl", "--bins", "1000"])
    assert a.act_quant == "kl" and a.bins == 1000
    assert set(tensor_cali_extensions.registry) == {"kl"} and tensor_cali_extensions.registry["kl"] is find_clip_val_kl
    assert set(tensor_cali_dispatcher.registry) == {"minmax", "hist", "mse"}       # the reference's registry is what it was
    assert tensor_cali_extensions("no_such_algorithm", None, None) is None
    from dipoorlet_amd.platform_settings import platform_setting_table
    assert all(kl_levels(d) == 128 for d in platform_setting_table)


def test_binding_declares_the_entry_point():
    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 22 and "dpl_hist_kl" in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["dpl_hist_kl"][1]) == 10
