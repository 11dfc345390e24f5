"""GPU: `-A qmse` — the quantisation-MSE clip search (k_hist_qmse<grid> / k_hist_kl_pick through dpl_hist_qmse) against its
definition, the exact-integer statement of tests/qmse_model.py, from the kernel up to the CLI.  The reference has no such
algorithm: the model is the yardstick."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import kl_model as K
import qmse_model as M
from _cases import MINI_NET, mini_net_activations
from test_hist_kl import MiniGraph, _accumulators, _bits, _many_slots, _mini_args

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-9, 1e-12        # fp64 against fp64 (tests/test_hist_kl.py's bound): the summation order, about 1e-13
GRIDS = (("Linear", 8, 128), ("Float8E4M3FN", 8, 128))       # (qtype, bit_width, first): what -D trt / stpu and -D ocp_fp8 search


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _kernel_cases():
    """[(bins, [(name, h, gmin, gmax, degenerate)], [(qtype, bit_width, first)])]: the model's fixture tensors at 128 (first ==
    bins: a single candidate), 1000 (no multiple of 64; there also the 4-bit grid, top = 7) and 2048 bins on both grids, one
    histogram scaled to a total above 2^33, and 16384 bins (128 KB of LDS): two tensors on the integer grid, one on E4M3."""
    out = []
    tensors = {k: K.fixture_tensor(k) for k in K.KINDS}
    for bins in (128, 1000, 2048):
        rows = [(k,) + K.abs_hist(tensors[k], bins) + (k in K.DEGENERATE,) for k in K.KINDS]
        if bins == 2048:
            h, gmin, gmax = K.abs_hist(tensors["normal"], bins)
            assert int(h.sum()) * 16384 > 2 ** 33
            rows.append(("normal_x16384", h * 16384, gmin, gmax, False))
        out.append((bins, rows, GRIDS + ((("Linear", 4, 8),) if bins == 1000 else ())))
    out.append((16384, [(k,) + K.abs_hist(tensors[k], 16384) + (False,) for k in ("normal", "laplace")], GRIDS[:1]))
    out.append((16384, [("small",) + K.abs_hist(tensors["small"], 16384) + (False,)], GRIDS[1:]))
    return out


def test_kernel_against_the_model(dev):
    """Per case: +inf exactly where the model has it; elsewhere |err - model| <= 1e-9 |model| + 1e-12; best == i* (or, at most
    once over all cases, a candidate the model itself holds within that bound of i*: a near-tie — the model's own curves need
    the clause zero times, asserted here); given best, the fp32 clip is the model's bit for bit.  Constant and all-zero tensors
    are checked by clip only."""
    near_ties, worst = 0, 0.0
    for bins, rows, grids in _kernel_cases():
        acc = _accumulators(dev, np.stack([r[1] for r in rows]), [r[2] for r in rows], [r[3] for r in rows])
        for qtype, bit_width, first in grids:
            grid, top = M.grid_of(qtype, bit_width)
            clip, best, err = (t.cpu().numpy() for t in acc.hist_qmse(qtype, bit_width, first))
            assert err.shape == (len(rows), bins + 1) and err.dtype == np.float64 and best.dtype == np.int32
            for s, (name, h, gmin, gmax, degenerate) in enumerate(rows):
                want_clip, i_star, curve = M.qmse_clip(h, gmin, gmax, first, grid, top)
                tag = (name, bins, qtype, top)
                if degenerate:
                    assert np.array_equal(_bits(clip[s]), _bits(want_clip)), (tag, clip[s], want_clip)
                    continue
                fin = np.isfinite(curve)
                assert np.array_equal(np.isposinf(err[s]), ~fin) and not np.isnan(err[s]).any() and not fin[:first].any(), tag
                d = np.abs(err[s][fin] - curve[fin])
                bound = RTOL * np.abs(curve[fin]) + ATOL
                worst = max(worst, float((d / bound).max()))
                print(f"qmse {name} bins={bins} {qtype} top={top}: candidates {int(fin.sum())}, max err/bound {float((d / bound).max()):.3g}, "
                      f"max abs err {float(d.max()):.3g}, i*={i_star} best={int(best[s])} min={curve[i_star]:.6g}")
                assert np.all(d <= bound), (tag, float(d.max()), int(np.argmax(d / bound)))
                # the model alone does not need the near-tie clause on this case
                others = np.delete(curve, i_star)
                if others.size:
                    assert others.min() > curve[i_star] * (1 + RTOL) + ATOL, (tag, float(others.min() - curve[i_star]))
                b = int(best[s])
                if b != i_star:
                    assert first <= b <= bins and curve[b] <= curve[i_star] * (1 + RTOL) + ATOL, (tag, b, i_star, curve[b], curve[i_star])
                    near_ties += 1
                assert np.array_equal(_bits(clip[s]), _bits(K.kl_clip_from_best(b, gmin, gmax, bins))), (tag, clip[s])
    print(f"qmse: worst err/bound {worst:.3g}, near-ties used {near_ties}")
    assert near_ties <= 1, near_ties


def test_empty_histogram_and_bad_arguments(dev):
    from dipoorlet_amd import _hip, ops
    acc = _accumulators(dev, np.zeros((2, 256), np.int64), [-1.5, -2.0], [2.5, 1.0])
    acc.hist[1, 255] = 4096                      # everything in the last bin: keep all, error 0
    for qtype, bit_width, first in GRIDS:
        clip, best, err = (t.cpu().numpy() for t in acc.hist_qmse(qtype, bit_width, first))
        assert best[0] == -1 and np.all(np.isposinf(err[0])) and np.array_equal(clip[0], np.array([-1.5, 2.5], np.float32))
        assert best[1] == 256 and err[1][256] == 0.0 and np.all(np.isposinf(err[1][:first])) and np.all(err[1][first:256] > 0)
        assert np.array_equal(_bits(clip[1]), _bits(K.kl_clip_from_best(256, -2.0, 1.0, 256)))
    small = _accumulators(dev, np.ones((1, 64), np.int64), [-1.0], [1.0])
    with pytest.raises(_hip.DipoorletHipError):
        small.hist_qmse("Linear", 8, 128)        # first > bins
    with pytest.raises(_hip.DipoorletHipError):
        small.hist_qmse("Float8E5M2", 8, 32)
    # the C ABI itself: status and message, nothing launched
    out = torch.full((1, 2), 7.0, dtype=torch.float32, device=dev)
    b = torch.full((1,), -7, dtype=torch.int32, device=dev)
    d = torch.full((65,), -7.0, dtype=torch.float64, device=dev)
    L = _hip.lib()
    head = (ops._ptr(small.hist), ops._ptr(small.gmin), ops._ptr(small.gmax), 1)
    tail = (ops._ptr(d), ops._ptr(b), ops._ptr(out), ops._stream())
    for bins, first, grid, top, word in ((64, 65, 0, 127, b"first"), (64, 0, 0, 127, b"first"), (64, 32, 2, 127, b"grid"),
                                         (64, 32, -1, 127, b"grid"), (64, 32, 0, 0, b"top"), (64, 32, 0, 32768, b"top"),
                                         (64, 32, 1, 448, b"top"), (0, 1, 0, 127, b"bins"), (_hip.MAX_BINS + 1, 32, 0, 127, b"bins")):
        assert L.dpl_hist_qmse(*head, bins, first, grid, top, *tail) != 0, (bins, first, grid, top)
        assert word in L.dpl_last_error(), (word, L.dpl_last_error())
    torch.cuda.synchronize()
    assert b.item() == -7 and (d == -7.0).all() and (out == 7.0).all()
    assert L.dpl_hist_qmse(*head, 64, 64, 0, 32767, *tail) == 0      # first == bins, the largest top
    assert L.dpl_hist_qmse(*head, 64, 1, 1, 0, *tail) == 0           # first == 1 on E4M3
    torch.cuda.synchronize()
    assert 1 <= b.item() <= 64 and torch.isfinite(d[1:]).all() and torch.isposinf(d[0])


def test_two_calls_same_bits_and_one_launch_equals_one_launch_per_slot(dev):
    """No floating-point atomics, a fixed reduction tree, and a candidate's value independent of the launch's geometry (123
    slots: 9 candidate chunks per tensor; one slot: 240)."""
    hs, lo, hi = _many_slots()
    acc = _accumulators(dev, hs, lo, hi)
    for qtype, bit_width, first in GRIDS:
        c1, b1, e1 = acc.hist_qmse(qtype, bit_width, first)
        c2, b2, e2 = acc.hist_qmse(qtype, bit_width, first)
        assert torch.equal(e1, e2) and torch.equal(b1, b2) and torch.equal(c1, c2)
        assert (b1 >= first).all() and torch.isfinite(e1[:, first:]).all()
        for s in range(hs.shape[0]):
            one = _accumulators(dev, hs[s:s + 1], lo[s:s + 1], hi[s:s + 1])
            c, b, e = one.hist_qmse(qtype, bit_width, first)
            assert torch.equal(e[0], e1[s]) and torch.equal(b[0], b1[s]) and torch.equal(c[0], c1[s]), (qtype, s)


def test_torch_op_equals_the_accumulator_method_and_refuses_cpu(dev):
    import dipoorlet_amd.torch_ops  # noqa: F401
    hs, lo, hi = _many_slots(n=6, bins=1000)
    acc = _accumulators(dev, hs, lo, hi)
    for qtype, bit_width, first in GRIDS + (("Linear", 4, 8),):
        clip = acc.hist_qmse(qtype, bit_width, first)[0]
        for s in range(hs.shape[0]):
            one = torch.ops.dipoorlet.hist_qmse(acc.hist[s].contiguous(), float(lo[s]), float(hi[s]), qtype, bit_width, first)
            assert one.shape == (2,) and one.dtype == torch.float32 and torch.equal(one, clip[s]), (qtype, bit_width, s)
    with pytest.raises(NotImplementedError):
        torch.ops.dipoorlet.hist_qmse(torch.zeros(256, dtype=torch.int64), -1.0, 1.0, "Linear", 8, 128)


# ------------------------------------------------------------------------------------------------ end to end: the API
@pytest.mark.parametrize("deploy", ["trt", "ocp_fp8"])
def test_find_clip_val_qmse_end_to_end(dev, tmp_path, monkeypatch, deploy):
    """find_clip_val_qmse on the MINI_NET set: the same clips at every batch size and without resident activations, equal to
    the model applied to the run's own histograms (the counts themselves are held bit-exact elsewhere), and the same again
    through the store_stats hook."""
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.tensor_cali import basic_algorithm as BA
    from dipoorlet_amd.tensor_cali import find_clip_val_qmse
    os.makedirs(tmp_path / "input")
    for i in range(8):
        mini_net_activations(i)[0][1].tofile(tmp_path / "input" / f"{i}.bin")
    seen = []
    orig = BA._hist_statistics

    def spy(*a, **k):
        acc, names = orig(*a, **k)
        seen.append((acc.hist.cpu().numpy().copy(), acc.gmin.cpu().numpy().copy(), acc.gmax.cpu().numpy().copy(), list(names)))
        return acc, names
    monkeypatch.setattr(BA, "_hist_statistics", spy)
    qi = platform_setting_table[deploy]["qi_params"]
    grid, top = M.grid_of(qi["type"], qi["bit_width"])
    first = find_clip_val_qmse(MiniGraph(), _mini_args(str(tmp_path), deploy=deploy, act_quant="qmse"))
    hist, gmin, gmax, names = seen[0]
    assert names == [n for n, _, _ in MINI_NET] and hasattr(first["conv1"][0], "tolist")
    for t, n in enumerate(names):
        want, i_star, curve = M.qmse_clip(hist[t], gmin[t], gmax[t], 128, grid, top)
        print(f"qmse e2e {deploy} {n}: i*={i_star} clip={want} total={int(hist[t].sum())}")
        assert np.array_equal(_bits(first[n]), _bits(want)), (n, first[n], want, i_star)
    for kw in (dict(calib_batch=1), dict(calib_batch=8), dict(resident_gb=0.0)):
        got = find_clip_val_qmse(MiniGraph(), _mini_args(str(tmp_path), deploy=deploy, act_quant="qmse", **kw))
        assert np.array_equal(seen[-1][0], hist), kw
        for n in names:
            assert np.array_equal(_bits(got[n]), _bits(first[n])), (kw, n)
    stats = {"minmax": {n: {"min": [gmin[t]], "max": [gmax[t]]} for t, n in enumerate(names)},
             "hist": {n: hist[t] for t, n in enumerate(names)}}
    got = find_clip_val_qmse(None, types.SimpleNamespace(bins=2048, deploy=deploy), store_stats=stats)
    for n in names:
        assert np.array_equal(_bits(got[n]), _bits(first[n])), n
    with pytest.raises(ValueError):
        find_clip_val_qmse(MiniGraph(), _mini_args(str(tmp_path), deploy=deploy, act_quant="qmse", bins=64))


# ------------------------------------------------------------------------------------------------ end to end: the CLI
N_IMG, BATCH, IMG = 8, 4, 64
CHILD_TIMEOUT_S = 600


def _cli(workdir, out, deploy):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "DPL_DIST_BACKEND")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["DPL_DETERMINISTIC"] = "1"      # (the library's deterministic convolutions: the runs compared here are separate processes)
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "model.onnx"), "-I",
           str(workdir / "calib"), "-N", str(N_IMG), "-A", "qmse", "-D", deploy, "-O", str(out), "--calib_batch", str(BATCH), "--skip_profiling"]
    return subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.mark.two_forwards
def test_cli_qmse_equals_the_api_and_refuses_an_asymmetric_platform(tmp_path):
    """Every child is a fresh process under its own `timeout`; a failing child ends the test, nothing is retried."""
    from dipoorlet_amd import dist_helper, models
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    g = models.resnet18(seed=11, image=IMG)
    g.output_dir = str(tmp_path)
    g.save_onnx_model("model")
    os.makedirs(tmp_path / "calib" / "input")
    rng = np.random.default_rng(5)
    for i in range(N_IMG):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(tmp_path / "calib" / "input" / f"{i}.bin")
    # refused before any device work: no process group, no output directory
    child = _cli(tmp_path, tmp_path / "refused", "snpe")
    text = child.communicate()[0]
    assert child.returncode not in (0, 124, 137), text[-3000:]
    assert "-A qmse is not supported with -D snpe" in text and "asymmetric" in text, text[-3000:]
    assert not os.path.exists(tmp_path / "refused")
    dist_helper.init_default()
    results = {}
    for deploy in ("trt", "ocp_fp8"):
        child = _cli(tmp_path, tmp_path / deploy, deploy)
        text = child.communicate()[0]
        assert child.returncode == 0, text[-3000:]
        act = json.load(open(tmp_path / deploy / "act_clip_val.json"))
        assert os.path.exists(tmp_path / deploy / {"trt": "trt_clip_val.json", "ocp_fp8": "ocp_fp8_scales.json"}[deploy]) and len(act) == 50
        # the API, in this process, on the same files
        args = types.SimpleNamespace(input_dir=str(tmp_path / "calib"), data_num=N_IMG, rank=0, local_rank=0, world_size=1, bins=2048,
                                     threshold=0.99999, deploy=deploy, act_quant="qmse", calib_batch=BATCH, merge="allreduce",
                                     optim_transformer=False)
        api, _ = tensor_calibration(ONNXGraph.load(str(tmp_path / "model.onnx")), args)
        assert set(api) == set(act)
        for n, v in api.items():
            assert act[n] == [float(v[0]), float(v[1])], (deploy, n, act[n], v)
        results[deploy] = act
    assert results["trt"] != results["ocp_fp8"]      # the grid decides: the same histograms, another answer
