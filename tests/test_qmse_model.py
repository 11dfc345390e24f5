"""CPU: the definition of `-A qmse` (tests/qmse_model.py) — its two statements agree, its minimum is no near-tie, the
degenerate histograms end where they must, and the host layers know the new key without the older registries having changed."""
import types

import numpy as np
import pytest

import kl_model as K
import qmse_model as M

BINS = (128, 1000, 2048)
GRIDS = ((M.UNIFORM, 127, 128), (M.E4M3, 448, 128), (M.UNIFORM, 7, 8))      # (grid, top, first)


@pytest.fixture(scope="module")
def curves():
    """{(kind, bins, grid, top): (h, first, curve by statement (a))}."""
    out = {}
    for kind in K.KINDS:
        x = K.fixture_tensor(kind)
        for bins in BINS:
            h = K.abs_hist(x, bins)[0]
            for grid, top, first in GRIDS:
                out[kind, bins, grid, top] = (h, first, M.qmse_curve(h, first, grid, top))
    return out


def test_two_statements_of_the_model_agree(curves):
    worst = 0.0
    for (kind, bins, grid, top), (h, first, a) in curves.items():
        b = M.qmse_curve_fp64(h, first, grid, top)
        assert a.shape == b.shape == (bins + 1,)
        assert np.all(np.isposinf(a[:first])) and np.all(np.isposinf(b[:first])), (kind, bins, grid, top)
        assert np.all(np.isfinite(a[first:])) and np.all(np.isfinite(b[first:])) and np.all(a[first:] >= 0), (kind, bins, grid, top)
        err, bound = np.abs(a[first:] - b[first:]), 1e-12 * np.abs(a[first:]) + 1e-12
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (kind, bins, grid, top, float((err / bound).max()))
        assert K.kl_best(a) == K.kl_best(b), (kind, bins, grid, top)
    print(f"qmse model: (a) against (b), worst err/bound {worst:.3g}")


def test_the_minimum_is_not_a_near_tie(curves):
    """The kernel test allows `best` to differ from i* where the model itself cannot tell two candidates apart (within
    1e-9 relative + 1e-12): on these tensors it can, by an order of magnitude and more — the closest pair lies 4.5e-6 relative
    apart (heavy_zero on E4M3, 2048 bins); fp64 summation noise is 1e-13."""
    closest = np.inf
    for (kind, bins, grid, top), (_, first, curve) in curves.items():
        if kind in K.DEGENERATE or top == 7 or bins == first:
            continue
        best = K.kl_best(curve)
        gap = np.delete(curve, best).min() - curve[best]
        closest = min(closest, gap / curve[best])
        assert gap > 10 * (1e-9 * abs(curve[best]) + 1e-12), (kind, bins, grid, gap, curve[best])
    print(f"qmse model: closest runner-up, relative {closest:.3g}")


def test_the_search_clips_where_the_definition_says(curves):
    """The integer grid clips harder than the 0.99999 percentile on every bell; E4M3, whose precision is relative, stays in the
    top octave of the range."""
    for kind in ("normal", "relu", "laplace", "outliers", "lognormal"):
        h = curves[kind, 2048, M.UNIFORM, 127][0]
        pct = int(np.argmax(np.cumsum(h) / h.sum() >= 0.99999)) + 1
        assert 128 <= K.kl_best(curves[kind, 2048, M.UNIFORM, 127][2]) < pct, kind
        assert K.kl_best(curves[kind, 2048, M.E4M3, 448][2]) > 1024, kind
    want = {"normal": (1657, 1963), "relu": (1649, 2009), "laplace": (1307, 2048), "outliers": (1269, 2015),
            "lognormal": (1334, 2020), "uniform": (2042, 1997)}
    for kind, (iu, ie) in want.items():
        assert (K.kl_best(curves[kind, 2048, M.UNIFORM, 127][2]), K.kl_best(curves[kind, 2048, M.E4M3, 448][2])) == (iu, ie), kind


def test_constant_tensor_keeps_all_with_error_zero_and_an_empty_histogram_has_no_best(curves):
    for bins in BINS:
        for grid, top, _ in GRIDS:
            curve = curves["constant", bins, grid, top][2]      # everything in the last bin: its centre is the clip of i = bins
            assert K.kl_best(curve) == bins and curve[bins] == 0.0, (bins, grid, top)
    for grid, top, first in GRIDS:
        clip, best, curve = M.qmse_clip(np.zeros(256, np.int64), -1.5, 2.5, first, grid, top)
        assert best == -1 and np.all(np.isposinf(curve)) and np.array_equal(clip, np.array([-1.5, 2.5], np.float32))
        assert np.all(np.isposinf(M.qmse_curve_fp64(np.zeros(256, np.int64), first, grid, top)))
    assert M.grid_of("Linear", 8) == (M.UNIFORM, 127) and M.grid_of("Linear", 4) == (M.UNIFORM, 7)
    assert M.grid_of("Float8E4M3FN") == (M.E4M3, 448)


def _parse(*argv):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "x", "-N", "8", *argv])


def test_cli_and_registries_know_qmse():
    from dipoorlet_amd.__main__ import check_args
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.tensor_cali import (find_clip_val_qmse, tensor_cali_dispatcher, tensor_cali_extensions,
                                           tensor_cali_grid_aware)
    a = _parse("-D", "trt", "-A", "qmse", "--bins", "1000")
    assert a.act_quant == "qmse" and a.bins == 1000
    assert set(tensor_cali_grid_aware.registry) == {"qmse"} and tensor_cali_grid_aware.registry["qmse"] is find_clip_val_qmse
    assert set(tensor_cali_extensions.registry) == {"kl"}
    assert set(tensor_cali_dispatcher.registry) == {"minmax", "hist", "mse"}
    assert tensor_cali_grid_aware("no_such_algorithm", None, None) is None
    allowed = {"trt", "stpu", "ocp_fp8"}
    assert allowed < set(platform_setting_table) and len(platform_setting_table) == 9
    reasons = {"magicmind": "asymmetric", "rv": "asymmetric", "atlas": "asymmetric", "snpe": "asymmetric", "imx": "powers of two"}
    for deploy in platform_setting_table:
        args = _parse("-D", deploy, "-A", "qmse")
        if deploy in allowed:
            check_args(args)
            continue
        with pytest.raises(ValueError) as e:
            check_args(args)
        assert f"-D {deploy}" in str(e.value) and "-A qmse" in str(e.value), str(e.value)
        if deploy in reasons:
            assert reasons[deploy] in str(e.value), str(e.value)
        else:       # ti: power-of-two scales and a dynamic sign, either is reason enough
            assert "powers of two" in str(e.value) or "dynamic_sym" in str(e.value)
    # the FP8 refusals are what they were, and name the new search among what works
    with pytest.raises(ValueError) as e:
        check_args(_parse("-D", "ocp_fp8", "-A", "kl"))
    assert "Supported: -A minmax, -A hist, -A qmse" in str(e.value)
    with pytest.raises(ValueError):
        check_args(_parse("-D", "ocp_fp8", "-A", "mse"))
    with pytest.raises(ValueError):
        check_args(_parse("-D", "ocp_fp8", "-A", "qmse", "--adaround"))


def test_find_clip_val_qmse_refuses_too_few_bins_before_any_device_work():
    from dipoorlet_amd.tensor_cali import find_clip_val_qmse
    for deploy in ("trt", "ocp_fp8"):
        with pytest.raises(ValueError) as e:
            find_clip_val_qmse(None, types.SimpleNamespace(bins=64, deploy=deploy))
        assert "--bins >= 128" in str(e.value)


def test_binding_declares_the_entry_point():
    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 25 and "dpl_hist_qmse" in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["dpl_hist_qmse"][1]) == 12
    assert (_hip.GRID_UNIFORM, _hip.GRID_E4M3) == (0, 1)


def test_bad_arguments_are_refused_on_the_host():
    """The C entry point checks its arguments before it touches the device: status and message without a GPU."""
    from dipoorlet_amd import _hip
    from dipoorlet_amd.csrc import build as hipbuild
    hipbuild.build()
    L = _hip.lib()
    for bins, first, grid, top, word in ((64, 65, 0, 127, b"first"), (64, 0, 0, 127, b"first"), (64, 32, 2, 127, b"grid"),
                                         (64, 32, 0, 0, b"top"), (64, 32, 0, 32768, b"top"), (64, 32, 1, 448, b"top"),
                                         (0, 1, 0, 127, b"bins"), (_hip.MAX_BINS + 1, 32, 0, 127, b"bins")):
        assert L.dpl_hist_qmse(None, None, None, 1, bins, first, grid, top, None, None, None, None) != 0, (bins, first, grid, top)
        assert word in L.dpl_last_error(), (word, L.dpl_last_error())
    assert L.dpl_hist_qmse(None, None, None, 0, 64, 32, 0, 127, None, None, None, None) == 0       # no slots: nothing to do
