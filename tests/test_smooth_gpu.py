"""GPU: k_colwise_absmax (dpl_colwise_absmax, ops.colwise_absmax, torch.ops.dipoorlet.colwise_absmax) bit for bit against its
definition np.maximum(acc, np.abs(x).max(0)) (tests/smooth_model.py; any NaN equal to any NaN), and `--smooth` end to end: the
statistics sweep, the effect on a fake-quantised mini-ViT with planted outlier channels, the CLI, two ranks."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import smooth_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, IMG = 8, 32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _zeros(c):
    return np.zeros(c, np.float32)


def _absmax(x, dev, acc=None):
    from dipoorlet_amd import ops
    out = ops.colwise_absmax(torch.from_numpy(x).to(dev), None if acc is None else torch.from_numpy(acc).to(dev))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. shapes
# (1100000, 8) and (530000, 3) are this file's own: a workgroup of the 16-byte kernel walks 4 * 256 / tw rows per trip (tw = lanes
# along the columns), so at 8 columns (tw = 2) the 2048-workgroup grid covers 1 048 576 rows in one trip and (70000, 8) makes one trip
# only; these two make a second trip in the 16-byte and in the scalar kernel.
SHAPES = [(1, 1), (3, 5), (394, 64), (7, 768), (50, 66), (70000, 8), (1000, 3072), (1100000, 8), (530000, 3), (300, 260), (5, 4100)]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_shapes(dev, rows, cols):
    x = np.random.default_rng(rows + cols).standard_normal((rows, cols)).astype(np.float32)
    x[rows // 2, cols // 2] = -1e30       # the maximum by magnitude is a negative value somewhere in the middle
    x[rows - 1, cols - 1] = 7e30          # ... and the very last element counts
    got = _absmax(x, dev)
    assert got.shape == (cols,) and M.same_bits(got, M.colwise_absmax(_zeros(cols), x))


def test_misaligned_base_and_rank_3(dev):
    from dipoorlet_amd import ops
    x = np.random.default_rng(1).standard_normal((394, 64)).astype(np.float32)
    buf = torch.zeros(394 * 64 + 1, device=dev)
    buf[1:] = torch.from_numpy(x).reshape(-1).to(dev)
    view = buf[1:].view(394, 64)              # contiguous, 4 bytes off a 16-byte boundary: the scalar kernel
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    assert M.same_bits(ops.colwise_absmax(view).cpu().numpy(), M.colwise_absmax(_zeros(64), x))
    x3 = np.random.default_rng(2).standard_normal((2, 197, 64)).astype(np.float32)
    assert M.same_bits(_absmax(x3, dev), M.colwise_absmax(_zeros(64), x3))
    x1 = np.random.default_rng(3).standard_normal(12).astype(np.float32)      # rank 1: one row
    assert M.same_bits(_absmax(x1, dev), np.abs(x1))


# ------------------------------------------------------------------------------------------------ 2. running accumulation
def test_running_accumulation(dev):
    from dipoorlet_amd import ops
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((100, 20)).astype(np.float32), (3 * rng.standard_normal((33, 20))).astype(np.float32)
    acc = ops.colwise_absmax(torch.from_numpy(a).to(dev))
    ret = ops.colwise_absmax(torch.from_numpy(b).to(dev), acc)
    assert ret is acc
    assert M.same_bits(acc.cpu().numpy(), M.colwise_absmax(M.colwise_absmax(_zeros(20), a), b))
    start = np.where(np.arange(20) % 3 == 0, np.float32(9.0), np.float32(0.01)).astype(np.float32)
    got = _absmax(a, dev, start.copy())
    assert M.same_bits(got, M.colwise_absmax(start, a)) and (got[::3] == 9.0).all() and (got[1::3] < 9.0).all()   # kept where larger
    keep = torch.from_numpy(start.copy()).to(dev)
    ops.colwise_absmax(torch.empty(0, 20, device=dev), keep)                                   # rows == 0: untouched
    assert np.array_equal(keep.cpu().numpy(), start)


# ------------------------------------------------------------------------------------------------ 3. special values
@pytest.mark.parametrize("misaligned", [False, True])
def test_special_values(dev, misaligned):
    from dipoorlet_amd import ops
    rows, cols = 37, 12
    x = np.random.default_rng(6).standard_normal((rows, cols)).astype(np.float32)
    x[20, 2] = np.nan
    x[5, 4] = -np.inf
    x[:, 6] = -0.0
    x[:, 8] = 0.0
    x[11, 8] = -1e-40                        # an fp32 subnormal
    x.view(np.uint32)[3, 10] = 0xFFC00001    # a negative NaN with a payload
    start = _zeros(cols)
    start[0] = np.nan                        # NaN already in acc
    if misaligned:
        buf = torch.zeros(rows * cols + 1, device=dev)
        buf[1:] = torch.from_numpy(x).reshape(-1).to(dev)
        xd = buf[1:].view(rows, cols)
    else:
        xd = torch.from_numpy(x).to(dev)
    got = ops.colwise_absmax(xd, torch.from_numpy(start).to(dev)).cpu().numpy()
    with np.errstate(invalid="ignore"):
        ref = M.colwise_absmax(start, x)
    assert M.same_bits(got, ref)             # (the neighbours of every special column included)
    assert np.isnan(got[0]) and np.isnan(got[2]) and np.isnan(got[10]) and got[4] == np.inf
    assert got[6] == 0 and got.view(np.uint32)[6] == 0                       # -0.0 counts as +0.0: no sign bit
    assert got[8] == np.float32(1e-40) and got[8] > 0
    assert np.isfinite(got[[1, 3, 5, 7, 9, 11]]).all()


# ------------------------------------------------------------------------------------------------ 4. argument checks
def test_argument_checks_and_torch_op(dev):
    import dipoorlet_amd.torch_ops  # noqa: F401
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    x = torch.ones(3, 4, device=dev)
    acc = torch.zeros(4, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dpl_colwise_absmax(C.c_void_p(x.data_ptr()), 3, 0, C.c_void_p(acc.data_ptr()), stream) == -2
    assert b"cols" in lib.dpl_last_error()
    assert lib.dpl_colwise_absmax(C.c_void_p(x.data_ptr()), -1, 4, C.c_void_p(acc.data_ptr()), stream) == -2
    assert lib.dpl_colwise_absmax(None, 3, 4, C.c_void_p(acc.data_ptr()), stream) == -2
    assert b"null" in lib.dpl_last_error()
    assert lib.dpl_colwise_absmax(C.c_void_p(x.data_ptr()), 3, 4, None, stream) == -2
    assert lib.dpl_colwise_absmax(None, 0, 4, None, stream) == 0              # rows == 0: nothing to do
    torch.cuda.synchronize()
    assert acc.cpu().tolist() == [0, 0, 0, 0]
    with pytest.raises(_hip.DipoorletHipError):
        ops.colwise_absmax(torch.ones(8, 6, device=dev).t())                  # not contiguous: no silent copy
    with pytest.raises(_hip.DipoorletHipError):
        ops.colwise_absmax(x, torch.zeros(5, device=dev))                     # acc of the wrong length
    with pytest.raises(_hip.DipoorletHipError):
        ops.colwise_absmax(x.double())
    with pytest.raises(_hip.DipoorletHipError):
        ops.colwise_absmax(torch.ones(3, 4))                                  # no CPU path
    y = torch.from_numpy(np.random.default_rng(8).standard_normal((2, 50, 24)).astype(np.float32)).to(dev)
    assert torch.equal(torch.ops.dipoorlet.colwise_absmax(y), ops.colwise_absmax(y))
    yt = y.transpose(0, 1)                                                    # (the torch op makes its input contiguous, as its siblings do)
    assert torch.equal(torch.ops.dipoorlet.colwise_absmax(yt), ops.colwise_absmax(yt.contiguous()))


# ------------------------------------------------------------------------------------------------ the mini-ViT work directory
def _write_images(d):
    os.makedirs(os.path.join(d, "calib", "input"), exist_ok=True)
    rng = np.random.default_rng(9)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(os.path.join(d, "calib", "input", f"{i}.bin"))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("smooth")
    g = M.mini_vit()
    g.output_dir = str(d)
    g.save_onnx_model("vit")
    _write_images(str(d))
    return d


def _args(workdir, out, deploy, **kw):
    os.makedirs(out, exist_ok=True)
    a = dict(model=str(workdir / "vit.onnx"), input_dir=str(workdir / "calib"), data_num=N, rank=0, local_rank=0, world_size=1,
             bins=2048, threshold=0.99999, deploy=deploy, act_quant="minmax", optim_transformer=False, merge="allreduce",
             calib_batch=4, output_dir=str(out), skip_layers=[], savefp=False, smooth_alpha=0.5)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _batches(workdir, graph, dev, chunk=4):
    from dipoorlet_amd.forward_net import load_input_batch
    shapes = {"input": graph.get_tensor_shape("input")}
    return [load_input_batch(str(workdir / "calib"), ["input"], shapes, i, i + chunk, dev)["input"] for i in range(0, N, chunk)]


# ------------------------------------------------------------------------------------------------ 5. the sweep
@pytest.mark.two_forwards
def test_sweep_equals_numpy_on_the_same_session(workdir, dev):
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.weight_transform.smooth import find_smooth_sites, smooth_statistics
    g = ONNXGraph.load(str(workdir / "vit.onnx"))
    sites = find_smooth_sites(g)
    assert len(sites) == 4
    sess = GraphSession(g, device=dev)
    got = smooth_statistics(g, sites, _args(workdir, workdir / "sweep", "trt"), session=sess)
    ref = M.site_statistics(sess, sites, _batches(workdir, g, dev))
    for s in sites:
        assert got[s.tensor].dtype == np.float32 and (ref[s.tensor] > 0).all()
        assert M.same_bits(got[s.tensor], ref[s.tensor]), s.gamma


# ------------------------------------------------------------------------------------------------ 6. the effect
def _output_error(g_fp, g_model, workdir, out, deploy, dev):
    """MSE of the fake-quantised `g_model` (its own -A minmax ranges) against the full-precision network `g_fp`, over the N images."""
    from dipoorlet_amd.quantize import quant_graph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    args = _args(workdir, out, deploy)
    act, wt = tensor_calibration(g_model, args)
    clip = {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**act, **wt}.items()}
    gq, _ = quant_graph(g_model, clip, args)
    x = torch.cat(_batches(workdir, g_fp, dev))
    fp = g_fp.make_session().run_named({"input": x}, [g_fp.network_outputs[0]])[0]
    q = gq.make_session().run_named({"input": x}, [gq.network_outputs[0]])[0]
    return float(((fp - q) ** 2).mean())


@pytest.mark.two_forwards
def test_smoothing_lowers_the_quantisation_error(workdir, dev):
    """The mini-ViT with outliers planted on 4 channels of every site (factor 16), `-D magicmind` (8-bit per-tensor MatMul inputs),
    -A minmax ranges re-derived for each model: the output MSE against fp32 must drop, err_smooth < err_plain.  No ratio is fixed
    in advance; the measured ones are printed and quoted in DESIGN section 3i.  `ocp_fp8` is printed only: a floating-point grid
    keeps its relative precision across binades, so a smaller gain is expected."""
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.weight_transform.smooth import find_smooth_sites, smooth_quant
    g = ONNXGraph.load(str(workdir / "vit.onnx"))
    planted = M.plant_outliers(g, find_smooth_sites(g))
    ratios = {}
    for deploy in ("magicmind", "ocp_fp8"):
        for tag, net in (("planted", planted), ("plain", g)):
            out = workdir / f"effect_{deploy}_{tag}"
            smoothed = smooth_quant(net, _args(workdir, out, deploy))
            assert smoothed is not net and os.path.exists(out / "smooth_model.onnx")
            e0 = _output_error(net, net, workdir, out, deploy, dev)
            e1 = _output_error(net, smoothed, workdir, out, deploy, dev)
            ratios[deploy, tag] = (e1 / e0, e0, e1)
            print(f"--smooth on -D {deploy}, {tag} mini-ViT: output MSE {e0:.4g} -> {e1:.4g} (ratio {e1 / e0:.4f})")
    r, e0, e1 = ratios["magicmind", "planted"]
    assert e1 < e0, (e0, e1)


# ------------------------------------------------------------------------------------------------ 7. CLI
def _cli(workdir, out, *extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["DPL_DETERMINISTIC"] = "1"
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "vit.onnx"), "-I",
           str(workdir / "calib"), "-N", str(N), "-A", "hist", "-D", "trt", "-O", str(out), *extra, "--bc", "--skip_profiling",
           "--calib_batch", "4"]
    return subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.mark.two_forwards
def test_cli(workdir, dev):
    """`-A hist -D trt --smooth --bc`: the smoothed model is written, re-calibrated and bias-corrected.  The ranges in act_clip_val.json
    are `-A hist`'s: [max(-clip, min x), min(clip, max x)], clip = the centre of the first bin of the 2048-bin |x| histogram at
    which the cumulated share reaches 0.99999 — with 8 704 values per site tensor that is the bin of max |x|, so clip lies at most
    one bin (1 / 2048) below max |x|.  A site tensor's entry is held (1e-6 relative) to the `-A hist` range of that tensor taken
    in this process from smooth_model.onnx, and to min x / max x of an fp32 forward of smooth_model.onnx through that formula."""
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    from dipoorlet_amd.weight_transform.smooth import find_smooth_sites
    out = workdir / "cli_smooth"
    r = _cli(workdir, out, "--smooth")
    assert r.returncode == 0, r.stdout[-3000:]
    assert os.path.exists(out / "smooth_model.onnx") and os.path.exists(out / "update_bias_model.onnx")
    g0, gs = ONNXGraph.load(str(workdir / "vit.onnx")), ONNXGraph.load(str(out / "smooth_model.onnx"))
    sites = find_smooth_sites(gs)
    assert [s.gamma for s in sites] == [s.gamma for s in find_smooth_sites(g0)] and len(sites) == 4
    for s in sites:
        assert not np.array_equal(gs.get_initializer(s.gamma), g0.get_initializer(s.gamma))
    act = json.load(open(out / "act_clip_val.json"))
    x = torch.cat(_batches(workdir, g0, dev))
    names = [s.tensor for s in sites]
    t_new = GraphSession(gs, device=dev).run_named({"input": x}, names)
    t_old = GraphSession(g0, device=dev).run_named({"input": x}, names)
    hist_new, _ = tensor_calibration(gs, _args(workdir, workdir / "cli_ref_new", "trt", act_quant="hist"))
    hist_old, _ = tensor_calibration(g0, _args(workdir, workdir / "cli_ref_old", "trt", act_quant="hist"))
    for n, tn, to in zip(names, t_new, t_old):
        lo, hi = act[n]
        for got, want in ((lo, float(hist_new[n][0])), (hi, float(hist_new[n][1]))):
            assert abs(got - want) <= 1e-6 * abs(want), (n, got, want)
        xmin, xmax = float(tn.min()), float(tn.max())
        top = max(-xmin, xmax)
        print(f"{n}: range [{lo:.6g}, {hi:.6g}]; fp32 forward of smooth_model.onnx [{xmin:.6g}, {xmax:.6g}], "
              f"of the input model [{float(to.min()):.6g}, {float(to.max()):.6g}]")
        # clip lies in [top * (1 - 1 / bins), top]; the range is [max(-clip, min x), min(clip, max x)]
        eps, near = 1e-6, top * (1 - 1 / 2048)
        assert min(near, xmax) * (1 - eps) <= hi <= min(top, xmax) * (1 + eps), (n, hi, xmin, xmax)
        assert min(near, -xmin) * (1 - eps) <= -lo <= min(top, -xmin) * (1 + eps), (n, lo, xmin, xmax)
        old_lo, old_hi = float(hist_old[n][0]), float(hist_old[n][1])
        assert abs(hi - old_hi) > 1e-3 * hi or abs(lo - old_lo) > 1e-3 * -lo      # not the input model's range
    # without the flag: nothing of --smooth happens, and the ranges are those of the calibration alone
    out2 = workdir / "cli_plain"
    r = _cli(workdir, out2)
    assert r.returncode == 0, r.stdout[-3000:]
    assert not os.path.exists(out2 / "smooth_model.onnx") and os.path.exists(out2 / "update_bias_model.onnx")
    plain = json.load(open(out2 / "act_clip_val.json"))
    assert set(plain) == set(hist_old)
    for n, (lo, hi) in plain.items():
        assert lo == float(hist_old[n][0]) and hi == float(hist_old[n][1]), n


# ------------------------------------------------------------------------------------------------ 8. two ranks
def _worker(rank, world, port, wd):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      DPL_DIST_BACKEND="gloo", DPL_DETERMINISTIC="1")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.backends.cudnn.deterministic = True
    from dipoorlet_amd import dist_helper
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.weight_transform.smooth import apply_smooth, find_smooth_sites, smooth_statistics
    dist_helper.init_default()
    args = types.SimpleNamespace(input_dir=os.path.join(wd, "calib"), data_num=N, rank=rank, local_rank=0, world_size=world,
                                 calib_batch=4, output_dir=wd)
    g = ONNXGraph.load(os.path.join(wd, "vit.onnx"))
    sites = find_smooth_sites(g)
    _, scales = apply_smooth(g, sites, smooth_statistics(g, sites, args), 0.5)
    np.savez(os.path.join(wd, f"scales{rank}.npz"), **scales)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.two_forwards
def test_two_ranks_agree_with_one(workdir, tmp_path):
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.weight_transform.smooth import apply_smooth, find_smooth_sites, smooth_statistics
    g = ONNXGraph.load(str(workdir / "vit.onnx"))
    g.output_dir = str(tmp_path)
    g.save_onnx_model("vit")
    _write_images(str(tmp_path))
    port = 29400 + os.getpid() % 90
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = np.load(tmp_path / "scales0.npz"), np.load(tmp_path / "scales1.npz")
    sites = find_smooth_sites(g)
    args = types.SimpleNamespace(input_dir=str(tmp_path / "calib"), data_num=N, rank=0, local_rank=0, world_size=1, calib_batch=4)
    _, one = apply_smooth(g, sites, smooth_statistics(g, sites, args), 0.5)
    assert sorted(a.files) == sorted(one) and len(one) == 4
    for k in one:       # a maximum is order-free: the shards' maxima merge to the whole set's
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        assert np.array_equal(a[k].view(np.uint32), one[k].view(np.uint32)), k
