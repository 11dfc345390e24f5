"""GPU: `-A kl` — the entropy clip search (k_hist_kl / k_hist_kl_pick through dpl_hist_kl) against its definition, the fp64
numpy model of tests/kl_model.py, from the kernel up to the CLI.  The reference has no such algorithm: the model is the
yardstick."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import kl_model as M
from _cases import MINI_NET, mini_net_activations

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-9, 1e-12        # fp64 against fp64, only the summation order differs (the model's own two statements: 1e-15)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _accumulators(dev, hists, gmins, gmaxs):
    """CalibAccumulators holding the given histograms ([n, bins] int64) and ranges."""
    from dipoorlet_amd import ops
    hists = np.ascontiguousarray(hists, np.int64)
    acc = ops.CalibAccumulators(hists.shape[0], dev, hists.shape[1])
    acc.set_minmax(torch.tensor(np.asarray(gmins, np.float32), device=dev), torch.tensor(np.asarray(gmaxs, np.float32), device=dev))
    acc.hist_prepare()
    acc.hist.copy_(torch.from_numpy(hists))
    return acc


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _kernel_cases():
    """[(bins, [(name, h, gmin, gmax, degenerate)])]: the model's fixture tensors at 128 / 1000 / 2048 bins, two of them at
    16384 bins, and one histogram scaled to a total above 2^33."""
    out = []
    tensors = {k: M.fixture_tensor(k) for k in M.KINDS}
    for bins in (128, 1000, 2048):
        rows = [(k,) + M.abs_hist(tensors[k], bins) + (k in M.DEGENERATE,) for k in M.KINDS]
        if bins == 2048:
            h, gmin, gmax = M.abs_hist(tensors["normal"], bins)
            assert int(h.sum()) * 16384 > 2 ** 33
            rows.append(("normal_x16384", h * 16384, gmin, gmax, False))
        out.append((bins, rows))
    out.append((16384, [(k,) + M.abs_hist(tensors[k], 16384) + (False,) for k in ("normal", "laplace")]))
    return out


def test_kernel_against_the_model(dev):
    """Per case: the admissible set is the model's; on it |div - model| <= 1e-9 |model| + 1e-12; best == i* (or, at most once
    over all cases, a candidate the model itself holds within that bound of i*: a near-tie — the model's own curves need the
    clause zero times, asserted here); given best, the fp32 clip is the model's bit for bit.  Constant and all-zero tensors
    (exact ties at 0) are checked by clip only."""
    near_ties, worst = 0, 0.0
    for bins, rows in _kernel_cases():
        acc = _accumulators(dev, np.stack([r[1] for r in rows]), [r[2] for r in rows], [r[3] for r in rows])
        for levels in (128, 32):
            if levels > bins or (bins == 16384 and levels == 128):        # (16384 bins: one level count — 4 s of model per case)
                continue
            clip, best, div = (t.cpu().numpy() for t in acc.hist_kl(levels))
            assert div.shape == (len(rows), bins + 1) and div.dtype == np.float64 and best.dtype == np.int32
            for s, (name, h, gmin, gmax, degenerate) in enumerate(rows):
                want_clip, i_star, curve = M.kl_clip(h, gmin, gmax, levels)
                tag = (name, bins, levels)
                if degenerate:
                    assert np.array_equal(_bits(clip[s]), _bits(want_clip)), (tag, clip[s], want_clip)
                    continue
                adm = np.isfinite(curve)
                assert np.array_equal(np.isfinite(div[s]), adm), (tag, int(adm.sum()), int(np.isfinite(div[s]).sum()))
                assert np.array_equal(np.isnan(div[s]), np.isnan(curve)) and np.all(np.isposinf(div[s][:levels])), tag
                err = np.abs(div[s][adm] - curve[adm])
                bound = RTOL * np.abs(curve[adm]) + ATOL
                worst = max(worst, float((err / bound).max()))
                print(f"kl {name} bins={bins} L={levels}: admissible {int(adm.sum())}, max err/bound {float((err / bound).max()):.3g}, "
                      f"max abs err {float(err.max()):.3g}, i*={i_star} best={int(best[s])} min={curve[i_star]:.6g}")
                assert np.all(err <= bound), (tag, float(err.max()), int(np.argmax(err / bound)))
                # the model alone does not need the near-tie clause on this case
                others = np.delete(np.where(np.isnan(curve), np.inf, curve), i_star)
                if others.size:
                    assert others.min() > curve[i_star] * (1 + RTOL) + ATOL, (tag, float(others.min() - curve[i_star]))
                b = int(best[s])
                if b != i_star:
                    assert 0 <= b <= bins and curve[b] <= curve[i_star] * (1 + RTOL) + ATOL, (tag, b, i_star, curve[b], curve[i_star])
                    near_ties += 1
                assert np.array_equal(_bits(clip[s]), _bits(M.kl_clip_from_best(b, gmin, gmax, bins))), (tag, clip[s])
    print(f"kl: worst err/bound {worst:.3g}, near-ties used {near_ties}")
    assert near_ties <= 1, near_ties


def test_empty_histogram_bad_levels_and_degenerate_range(dev):
    from dipoorlet_amd import _hip, ops
    acc = _accumulators(dev, np.zeros((2, 256), np.int64), [-1.5, 0.0], [2.5, 0.0])
    acc.hist[1, 128] = 4096                      # an all-zero tensor: range (0, 0), every element in the bin of |0|
    clip, best, div = (t.cpu().numpy() for t in acc.hist_kl(128))
    assert best[0] == -1 and np.all(np.isposinf(div[0])) and np.array_equal(clip[0], np.array([-1.5, 2.5], np.float32))
    assert best[1] == 129 and clip[1][0] == 0.0 and clip[1][1] == 0.0
    small = _accumulators(dev, np.ones((1, 64), np.int64), [-1.0], [1.0])
    with pytest.raises(_hip.DipoorletHipError):
        small.hist_kl(128)
    # the C ABI itself: status and message, nothing launched
    out = torch.empty(1, 2, dtype=torch.float32, device=dev)
    b = torch.empty(1, dtype=torch.int32, device=dev)
    d = torch.empty(65, dtype=torch.float64, device=dev)
    L = _hip.lib()
    args = (ops._ptr(small.hist), ops._ptr(small.gmin), ops._ptr(small.gmax), 1, 64)
    assert L.dpl_hist_kl(*args, 128, ops._ptr(d), ops._ptr(b), ops._ptr(out), ops._stream()) != 0
    assert b"levels" in L.dpl_last_error()
    assert L.dpl_hist_kl(*args, 1, ops._ptr(d), ops._ptr(b), ops._ptr(out), ops._stream()) != 0
    assert L.dpl_hist_kl(args[0], args[1], args[2], 1, _hip.MAX_BINS + 1, 128, ops._ptr(d), ops._ptr(b), ops._ptr(out), ops._stream()) != 0
    assert b"bins" in L.dpl_last_error()
    assert L.dpl_hist_kl(*args, 64, ops._ptr(d), ops._ptr(b), ops._ptr(out), ops._stream()) == 0      # levels == bins is allowed
    torch.cuda.synchronize()
    assert b.item() == 64


def _many_slots(n=123, bins=2048):
    rng = np.random.default_rng(77)
    hs, lo, hi = [], [], []
    for t in range(n):
        x = rng.standard_normal(20000 + 997 * t).astype(np.float32) * np.float32(0.5 + 0.05 * t)
        if t % 2:
            x = np.maximum(x, np.float32(0))
        h, gmin, gmax = M.abs_hist(x, bins)
        hs.append(h)
        lo.append(gmin)
        hi.append(gmax)
    return np.stack(hs), np.asarray(lo, np.float32), np.asarray(hi, np.float32)


def test_two_calls_same_bits_and_one_launch_equals_one_launch_per_slot(dev):
    """No floating-point atomics, a fixed reduction tree, and a candidate's value independent of the launch's geometry (123
    slots: 9 candidate chunks per tensor; one slot: 240)."""
    hs, lo, hi = _many_slots()
    acc = _accumulators(dev, hs, lo, hi)
    c1, b1, d1 = acc.hist_kl(128)
    c2, b2, d2 = acc.hist_kl(128)
    assert torch.equal(d1, d2) and torch.equal(b1, b2) and torch.equal(c1, c2)
    assert (b1 >= 128).all() and not torch.isnan(d1).any()
    for s in range(hs.shape[0]):
        one = _accumulators(dev, hs[s:s + 1], lo[s:s + 1], hi[s:s + 1])
        c, b, d = one.hist_kl(128)
        assert torch.equal(d[0], d1[s]) and torch.equal(b[0], b1[s]) and torch.equal(c[0], c1[s]), s


def test_torch_op_equals_the_accumulator_method_and_refuses_cpu(dev):
    import dipoorlet_amd.torch_ops  # noqa: F401
    hs, lo, hi = _many_slots(n=6, bins=1000)
    acc = _accumulators(dev, hs, lo, hi)
    for levels in (128, 32):
        clip = acc.hist_kl(levels)[0]
        for s in range(hs.shape[0]):
            one = torch.ops.dipoorlet.hist_kl(acc.hist[s].contiguous(), float(lo[s]), float(hi[s]), levels)
            assert one.shape == (2,) and one.dtype == torch.float32 and torch.equal(one, clip[s]), (levels, s)
    with pytest.raises(NotImplementedError):
        torch.ops.dipoorlet.hist_kl(torch.zeros(256, dtype=torch.int64), -1.0, 1.0, 128)


# ------------------------------------------------------------------------------------------------ end to end: the API
class MiniSession:
    """Plays the network: returns the prescribed activations of whichever images are in the batch."""

    def __init__(self, device):
        self.tensor_names = [n for n, _, _ in MINI_NET]
        self.elems_per_image = [e for _, e, _ in MINI_NET]
        self.device = device
        self.by_key = {}
        for i in range(8):
            acts = mini_net_activations(i)
            self.by_key[float(acts[0][1][0])] = acts

    def run(self, inputs):
        x = inputs["input"]
        b = x.shape[0]
        keys = x.reshape(b, -1)[:, 0].cpu().numpy()
        per = [self.by_key[float(k)] for k in keys]
        out = [x.reshape(b, -1).contiguous()]
        for t in range(1, len(MINI_NET)):
            out.append(torch.from_numpy(np.stack([p[t][1] for p in per])).to(self.device))
        return out


class MiniGraph:
    network_inputs = ["input"]

    def get_tensor_shape(self, name):
        return [1, 3, 32, 32]

    def make_session(self, args):
        return MiniSession(torch.device("cuda:0"))


def _mini_args(calib_dir, **kw):
    a = types.SimpleNamespace(input_dir=calib_dir, data_num=8, rank=0, local_rank=0, world_size=1, bins=2048, threshold=0.99999,
                              deploy="trt", act_quant="kl", optim_transformer=False, merge="allreduce", calib_batch=3)
    a.__dict__.update(kw)
    return a


def test_find_clip_val_kl_end_to_end(dev, tmp_path, monkeypatch):
    """find_clip_val_kl on the MINI_NET set: the same clips at every batch size and without resident activations, equal to the
    model applied to the run's own histograms (the counts themselves are held bit-exact elsewhere), and the same again through
    the store_stats hook."""
    from dipoorlet_amd.tensor_cali import basic_algorithm as BA
    from dipoorlet_amd.tensor_cali import find_clip_val_kl
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
    first = find_clip_val_kl(MiniGraph(), _mini_args(str(tmp_path)))
    hist, gmin, gmax, names = seen[0]
    assert names == [n for n, _, _ in MINI_NET] and hasattr(first["conv1"][0], "tolist")
    for t, n in enumerate(names):
        want, i_star, curve = M.kl_clip(hist[t], gmin[t], gmax[t], 128)
        print(f"kl e2e {n}: i*={i_star} clip={want} total={int(hist[t].sum())}")
        assert np.array_equal(_bits(first[n]), _bits(want)), (n, first[n], want, i_star)
    for kw in (dict(calib_batch=1), dict(calib_batch=8), dict(resident_gb=0.0)):
        got = find_clip_val_kl(MiniGraph(), _mini_args(str(tmp_path), **kw))
        assert np.array_equal(seen[-1][0], hist), kw
        for n in names:
            assert np.array_equal(_bits(got[n]), _bits(first[n])), (kw, n)
    stats = {"minmax": {n: {"min": [gmin[t]], "max": [gmax[t]]} for t, n in enumerate(names)},
             "hist": {n: hist[t] for t, n in enumerate(names)}}
    got = find_clip_val_kl(None, types.SimpleNamespace(bins=2048, deploy="trt"), store_stats=stats)
    for n in names:
        assert np.array_equal(_bits(got[n]), _bits(first[n])), n
    with pytest.raises(ValueError):
        find_clip_val_kl(MiniGraph(), _mini_args(str(tmp_path), bins=64))


# ------------------------------------------------------------------------------------------------ end to end: the CLI
N_IMG, BATCH, IMG = 8, 4, 64
CHILD_TIMEOUT_S = 600


def _cli(workdir, out, env_extra=None, port=None, rank=None, world=1):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "DPL_DIST_BACKEND")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["DPL_DETERMINISTIC"] = "1"      # (the library's deterministic convolutions: the runs compared here are separate processes)
    if rank is not None:
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), DPL_DIST_BACKEND="gloo")
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "model.onnx"), "-I",
           str(workdir / "calib"), "-N", str(N_IMG), "-A", "kl", "-D", "trt", "-O", str(out), "--calib_batch", str(BATCH), "--skip_profiling"]
    return subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _wait(children):
    """Every child is a fresh process under its own `timeout`; a failing child ends the test, nothing is retried."""
    outs = [c.communicate()[0] for c in children]
    for c, o in zip(children, outs):
        assert c.returncode == 0, o[-3000:]


@pytest.mark.two_forwards
def test_cli_kl_one_rank_equals_the_api_and_two_ranks_equal_one(tmp_path):
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
    _wait([_cli(tmp_path, tmp_path / "w1")])
    act = json.load(open(tmp_path / "w1" / "act_clip_val.json"))
    assert os.path.exists(tmp_path / "w1" / "trt_clip_val.json") and len(act) == 50
    # the API, in this process, on the same files
    dist_helper.init_default()
    args = types.SimpleNamespace(input_dir=str(tmp_path / "calib"), data_num=N_IMG, rank=0, local_rank=0, world_size=1, bins=2048,
                                 threshold=0.99999, deploy="trt", act_quant="kl", calib_batch=BATCH, merge="allreduce",
                                 optim_transformer=False)
    api, _ = tensor_calibration(ONNXGraph.load(str(tmp_path / "model.onnx")), args)
    assert set(api) == set(act)
    for n, v in api.items():
        assert act[n] == [float(v[0]), float(v[1])], (n, act[n], v)
    # two ranks on the one GPU (gloo): every rank searches the same all-reduced histogram
    port = 29800 + os.getpid() % 150
    _wait([_cli(tmp_path, tmp_path / "w2", port=port, rank=r, world=2) for r in range(2)])
    act2 = json.load(open(tmp_path / "w2" / "act_clip_val.json"))
    assert act2 == act
    for r in range(2):
        assert json.load(open(tmp_path / "w2" / f"act_clip_val.json.rank{r}")) == act
