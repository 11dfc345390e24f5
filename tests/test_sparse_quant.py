"""GPU: `--sparse` (sparse + quantised weights) against reference-generated vectors (tests/golden/round_level.*:
prune masks, quant_weight_wo_roundmask with its straight-through gradient, an SGD + cosine-LR trajectory) and end to
end through the CLI."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "round_level.npz"))
META = json.load(open(os.path.join(HERE, "golden", "round_level.json")))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def test_prune_masks_golden():
    from dipoorlet_amd.weight_transform.sparse_quant_layer import create_nv24_mask, create_unstruction_mask, prune_weight
    w4, w2 = dev(Z["sp_w4"]), dev(Z["sp_w2"])
    assert np.array_equal(create_unstruction_mask(w4, 0.5).cpu().numpy(), Z["sp_mask_unstr_w4"])
    assert np.array_equal(create_unstruction_mask(w2, 0.3).cpu().numpy(), Z["sp_mask_unstr_w2_30"])
    assert np.array_equal(create_nv24_mask(w4, 2, 4).cpu().numpy(), Z["sp_mask_nv24_w4"])
    assert np.array_equal(create_nv24_mask(w2, 2, 4).cpu().numpy(), Z["sp_mask_nv24_w2"])
    assert float(create_unstruction_mask(w4, 0.0).min()) == 1.0
    p = prune_weight(w4, {"pattern": "nv24", "rate": 0.5}).cpu().numpy()
    assert np.array_equal(p, Z["sp_w4"] * Z["sp_mask_nv24_w4"])


@pytest.mark.parametrize("row", META["sparse_quant"], ids=lambda r: r["key"])
def test_quantiser_value_and_straight_through_gradient(row):
    from dipoorlet_amd import _hip
    from dipoorlet_amd.ops import _ptr, _stream
    from dipoorlet_amd.weight_transform.sparse_quant_layer import create_unstruction_mask, quant_weight_wo_roundmask
    k = row["key"]
    w, G, scale = dev(Z[row["w"]]), dev(Z[k + "_G"]), dev(Z[k + "_scale"])
    qmin, qmax = torch.full_like(scale, -127.0), torch.full_like(scale, 127.0)
    mask = create_unstruction_mask(w, 0.5)
    qw = quant_weight_wo_roundmask(w, scale, qmin, qmax, row["per_channel"], mask=mask)
    np.testing.assert_allclose(qw.cpu().numpy(), Z[k + "_qw"], rtol=1e-6, atol=1e-9)
    g = torch.empty_like(w)
    wc = w.clone()
    nch = scale.numel()
    _hip.check(_hip.lib().dpl_sparse_step(_ptr(G), _ptr(wc), _ptr(mask), None, _ptr(scale), _ptr(qmin), _ptr(qmax),
                                          w.numel(), nch, w.numel() // nch, 1 if row["per_channel"] else 0, 1.0, 0.0, 0.0,
                                          0.0, 1, 0, _ptr(g), _stream()), "dpl_sparse_step")
    np.testing.assert_allclose(g.cpu().numpy(), Z[k + "_grad"], rtol=2e-6, atol=1e-9)
    assert torch.equal(wc, w)                                      # update = 0: nothing written
    if row["per_channel"]:                                         # the clamp was hit and blocks the gradient there
        sat = np.abs(Z[k + "_qw"] / Z[k + "_scale"].reshape(-1, 1, 1, 1)) >= 127.0 - 1e-3
        assert sat.any() and np.all(Z[k + "_grad"][sat & (np.abs(Z[row["w"]]) > 1.28 * Z[k + "_scale"].reshape(-1, 1, 1, 1) * 100)] == 0)


def test_sgd_trajectory_golden():
    from dipoorlet_amd.onnx_io import Node
    from dipoorlet_amd.weight_transform.reconstruction import learn_sparse
    from dipoorlet_amd.weight_transform.sparse_quant_layer import SparseQLayer, cosine_lr
    t = META["sparse_traj"]
    node = Node("Conv", ["x", "w", "b"], ["y"], name="c", attrs={"pads": [1, 1, 1, 1], "kernel_shape": [3, 3],
                                                                  "strides": [1, 1], "dilations": [1, 1], "group": 1})
    scale = dev(Z["sptraj_scale"])
    qw = {"scale": scale, "q_min": torch.full_like(scale, -127.0), "q_max": torch.full_like(scale, 127.0),
          "per_channel": True}
    layer = SparseQLayer(node, dev(Z["sptraj_w"]), dev(Z["sptraj_b"]), qw, True, {"pattern": "unstruction", "rate": t["rate"]})
    torch.backends.cudnn.allow_tf32 = False
    last = learn_sparse(layer, dev(Z["sptraj_x"]), dev(Z["sptraj_fp"]), t["bs"], t["epochs"])
    assert last == pytest.approx(Z["sptraj_losses"][-1], rel=2e-3)
    np.testing.assert_allclose(layer.weight.cpu().numpy(), Z["sptraj_learned"], rtol=0, atol=2e-5)
    final = layer.new_weight().cpu().numpy()
    assert np.mean(final == Z["sptraj_final"]) >= 0.99 and np.mean(final == 0.0) >= 0.5
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3), T_max=12)
    for ep in range(12):
        assert cosine_lr(1e-3, ep, 12) == pytest.approx(sched.get_last_lr()[0], rel=1e-12, abs=1e-18)
        sched.optimizer.step()
        sched.step()


def test_sparse_cli(tmp_path):
    from dipoorlet_amd import models
    from dipoorlet_amd.__main__ import main
    from dipoorlet_amd.graph import ONNXGraph
    d = str(tmp_path)
    g = models.resnet18(seed=4, image=32)
    g.output_dir = d
    g.save_onnx_model("model")
    os.makedirs(os.path.join(d, "calib", "input"))
    rng = np.random.default_rng(1)
    for i in range(8):
        rng.standard_normal(3 * 32 * 32).astype(np.float32).tofile(os.path.join(d, "calib", "input", f"{i}.bin"))
    out = os.path.join(d, "out")
    assert main(["-M", os.path.join(d, "model.onnx"), "-I", os.path.join(d, "calib"), "-N", "8", "-A", "minmax", "-D",
                 "trt", "-O", out, "--calib_batch", "8", "--skip_profiling", "--sparse", "--pattern", "nv24", "--ada_bs",
                 "8", "--ada_epoch", "3"]) == 0
    g1 = ONNXGraph.load(os.path.join(out, "sparse_quant.onnx"))
    checked = 0
    for node in g1.graph.node:
        if node.op_type == "Conv" and g1.get_initializer(node.input[1]).shape[1] % 4 == 0:
            w = g1.get_initializer(node.input[1])
            grp = np.abs(w).transpose(0, 2, 3, 1).reshape(-1, 4)
            assert np.all((grp != 0).sum(1) <= 2), node.name        # 2 : 4 along the input channels
            checked += 1
    assert checked >= 15 and os.path.exists(os.path.join(out, "trt_clip_val.json"))


# ====================================================================================================================
# dpl_sparse_quant / dpl_sparse_step through the C ABI against oracle/round_oracle.py (sparse_quant, sparse_grad, Sgd: pinned
# to the golden rows and to torch.optim.SGD in tests/test_round_oracle_golden.py), every output bit for bit: no transcendental
# is involved.  Sizes that take the grid-stride loops round a second time, and constructed edges.
import ctypes as C                                   # noqa: E402

import round_cases as RC                             # noqa: E402
from round_cases import assert_bits                  # noqa: E402

F32 = np.float32


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def host(t):
    return t.detach().cpu().numpy()


def _chan(d):
    n = d["w"].size
    nch = d["scale"].size
    return n, nch, n // nch


def _grid(d):
    """(scale, q_min, q_max) on the device, held by the case so that they outlive the launch that reads them."""
    if "_grid" not in d:
        d["_grid"] = tuple(dev(d[k]) for k in ("scale", "qmin", "qmax"))
    return d["_grid"]


def k_sparse_quant(d, w, mask):
    from dipoorlet_amd import _hip
    n, nch, inner = _chan(d)
    sc, lo, hi = _grid(d)
    out = torch.full_like(w, 777.0)
    _hip.check(_hip.lib().dpl_sparse_quant(_p(w), _p(mask), _p(sc), _p(lo), _p(hi), n, nch,
                                           inner, int(d["pc"]), _p(out), None), "dpl_sparse_quant")
    return out


def k_sparse_step(d, G, w, mask, buf, grad_scale=1.0, lr=1e-3, momentum=0.9, wd=1e-4, first=0, update=1, want_g=True):
    """dpl_sparse_step on device tensors (w and buf updated in place) -> grad_w."""
    from dipoorlet_amd import _hip
    n, nch, inner = _chan(d)
    sc, lo, hi = _grid(d)
    g = torch.full_like(w, 777.0) if want_g else None
    _hip.check(_hip.lib().dpl_sparse_step(_p(G), _p(w), _p(mask), _p(buf), _p(sc), _p(lo),
                                          _p(hi), n, nch, inner, int(d["pc"]), grad_scale, lr, momentum, wd,
                                          first, update, _p(g), None), "dpl_sparse_step")
    return g


@pytest.mark.parametrize("name", [r[0] for r in RC.LAYOUTS])
def test_sparse_kernels_second_trip_bit_exact(name):
    """Quantiser (with and without a prune mask) and two consecutive fused SGD steps per setting on arrays with n > 2^20 (and
    2^20 - 1, 2^20): the straight-through gradient, the momentum buffer and the weight of EVERY element bit for bit.  The
    first step starts from a buffer full of NaN (`first` must not read it); weight decay 0 takes the branch that skips the
    add; grad_scale 0.5 is a multi-rank run; the learning rates are two epochs of cosine_lr."""
    from oracle import round_oracle as ro
    from dipoorlet_amd.weight_transform.sparse_quant_layer import cosine_lr
    d = RC.layout_data(name)
    prune = dev(d["prune"])
    for mask_h, mask_d in ((d["prune"], prune), (None, None)):
        qw = host(k_sparse_quant(d, dev(d["w"]), mask_d))
        assert_bits(qw, ro.sparse_quant(d["w"], mask_h, d["scale"], d["qmin"], d["qmax"], d["pc"])[0], "qw")
    if d["pc"] and d["shape"][-1] != 1:
        assert (np.abs(qw / ro._bc(d["scale"], qw.ndim)) == 127).any()                  # the clamp was exercised
    for wd, gs in ((1e-4, 1.0), (0.0, 0.5)):
        w_h = d["w"].copy()
        w, buf = dev(w_h), torch.full_like(prune, float("nan"))
        sgd = ro.Sgd(1e-3, 0.9, wd)
        for it, G in enumerate((d["G"], d["G2"])):
            lr = cosine_lr(1e-3, 3 + 5 * it, 12)
            _, passf = ro.sparse_quant(w_h, d["prune"], d["scale"], d["qmin"], d["qmax"], d["pc"])
            want_g = ro.sparse_grad(G, d["prune"], d["scale"], passf, gs)
            g = k_sparse_step(d, dev(G), w, prune, buf, gs, lr, 0.9, wd, first=1 if it == 0 else 0)
            assert_bits(host(g), want_g, f"grad_w step {it + 1}")
            w_h = sgd.step(w_h, want_g, lr)
            assert_bits(host(buf), sgd.buf, f"momentum buffer step {it + 1}")
            assert_bits(host(w), w_h, f"weight step {it + 1}")
        assert not np.array_equal(w_h, d["w"])


def _edge(w, scale, qmin, qmax, pc=True):
    w = np.asarray(w, F32)
    return {"w": w, "scale": np.asarray(scale, F32).reshape(-1), "qmin": np.asarray(qmin, F32).reshape(-1),
            "qmax": np.asarray(qmax, F32).reshape(-1), "pc": pc, "shape": w.shape}


def test_sparse_rounding_ties_clamp_ties_zero_and_denormals():
    """Power-of-two scale, w = k * scale exactly.  rint is half to even (±0.5, ±1.5, ±2.5 scales), -0.0 and denormal weights
    quantise to zero.  The clamp's pass factor is directly visible in grad_w: 1 inside, 0.5 on rint(w / scale) == ±127
    exactly, 0 outside, never 0.25; per tensor nothing clamps."""
    from oracle import round_oracle as ro
    s = F32(2.0 ** -7)
    k = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0, 0.0, 126, 126.5, 127, 127.49, 127.5, 128, -126, -126.5, -127,
                  -127.49, -127.5, -128, 126.49, 1e6, -1e6], F32)
    w = np.concatenate([k * s, np.array([1e-40, -1e-40, 1.4e-45], F32)])
    rk = np.array([0, 0, 2, -2, 2, -2, 0, 0, 126, 126, 127, 127, 128, 128, -126, -126, -127, -127, -128, -128, 126, 1e6, -1e6,
                   0, 0, 0], F32)
    passf = np.array([1] * 8 + [1, 1, .5, .5, 0, 0, 1, 1, .5, .5, 0, 0, 1, 0, 0] + [1] * 3, F32)
    G = (np.arange(len(w), dtype=F32) + 2) / 8
    for pc in (True, False):
        d = _edge(w, [s], [-127], [127], pc)
        qw = host(k_sparse_quant(d, dev(w), None))
        assert_bits(qw, (np.clip(rk, -127, 127) if pc else rk) * s, f"qw pc={pc}")
        oq, op = ro.sparse_quant(w, None, [s], [-127], [127], pc)
        assert_bits(qw, oq, "qw / oracle")
        wd_, buf = dev(w), torch.zeros(len(w), device="cuda")
        g = host(k_sparse_step(d, dev(G), wd_, None, buf, update=0))
        assert_bits(g, G * (passf if pc else 1), f"grad_w pc={pc}")           # (G * s) * pass / s is exact for s = 2^-7
        assert_bits(g, ro.sparse_grad(G, None, [s], op), "grad_w / oracle")
        assert_bits(host(wd_), w, "update = 0 leaves the weight")
        assert not host(buf).any()


def test_sparse_step_first_garbage_buffer_and_weight_decay():
    """`first` takes buf = g whatever the buffer held (inf / NaN garbage); afterwards the buffer is read.  Weight decay enters
    the buffer and the weight, never grad_w; with weight decay 0 the add is skipped (w = inf would otherwise turn 0 * inf
    into NaN in the buffer)."""
    from oracle import round_oracle as ro
    rng = np.random.default_rng(9)
    w0 = rng.standard_normal(1000).astype(F32)
    G = rng.standard_normal(1000).astype(F32)
    d = _edge(w0, [2.0 ** -6], [-127], [127], pc=False)
    garbage = np.resize(np.array([np.nan, np.inf, -np.inf, 1e38, -3.0], F32), 1000)
    for wd in (0.0, 1e-4, 0.5):
        w, buf = dev(w0), dev(garbage)
        sgd = ro.Sgd(1e-2, 0.9, wd)
        g = host(k_sparse_step(d, dev(G), w, None, buf, 1.0, 1e-2, 0.9, wd, first=1))
        assert_bits(g, G, "grad_w carries no weight decay")               # per tensor, s = 2^-6: (G * s) / s is exact
        w1 = sgd.step(w0, G, 1e-2)
        assert_bits(host(buf), sgd.buf, "first: buf = g (+ wd * w)")
        assert_bits(host(w), w1, "w")
        assert np.isfinite(host(buf)).all()
        g = host(k_sparse_step(d, dev(G), w, None, buf, 1.0, 1e-2, 0.9, wd, first=0))
        w2 = sgd.step(w1, G, 1e-2)
        assert_bits(host(buf), sgd.buf, "second: momentum * buf + g")
        assert_bits(host(w), w2, "w after the second step")
        assert wd == 0 or not np.array_equal(sgd.buf, (G * F32(0.9) + G).astype(F32))
    winf = w0.copy()
    winf[5] = np.inf
    w, buf = dev(winf), dev(garbage)
    k_sparse_step(d, dev(G), w, None, buf, 1.0, 1e-2, 0.9, 0.0, first=1)
    assert host(buf)[5] == G[5] and host(w)[5] == np.inf


@pytest.mark.parametrize("name,d", RC.special_cases(("w", "G")), ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("pc", (True, False))
def test_sparse_kernels_keep_a_special_value_in_its_element(name, d, pc):
    """One NaN / ±inf in the weight or the upstream gradient: qw, grad_w, the buffer and the weight bit for bit as the oracle
    (pinned to torch autograd on these rows) has them — a NaN weight quantises to NaN and, as in torch.max / torch.min's
    backward, lets the straight-through gradient pass — and no other element differs from the run without it."""
    from oracle import round_oracle as ro
    sc = d["scale"] if pc else d["scale"][:1]
    outs = {}
    for key, c in (("case", d), ("base", RC.special_base())):
        e = _edge(c["w"], sc, c["qmin"][:len(sc)], c["qmax"][:len(sc)], pc)
        w, buf, prune = dev(c["w"]), torch.full((2, 8), float("nan"), device="cuda"), dev(c["prune"])
        qw = k_sparse_quant(e, w, prune)
        g = k_sparse_step(e, dev(c["G"]), w, prune, buf, 1.0, 1e-3, 0.9, 1e-4, first=1)
        outs[key] = [host(t) for t in (qw, g, buf, w)]
        if key == "case":
            oq, passf = ro.sparse_quant(c["w"], c["prune"], sc, e["qmin"], e["qmax"], pc)
            og = ro.sparse_grad(c["G"], c["prune"], sc, passf)
            sgd = ro.Sgd(1e-3, 0.9, 1e-4)
            ow = sgd.step(c["w"], og, 1e-3)
            for got, want, what in zip(outs[key], (oq, og, sgd.buf, ow), ("qw", "grad_w", "buf", "w")):
                assert_bits(got, want, (name, what))
    if name.endswith("nan"):
        for i in (0, 2, 3) if name.startswith("w") else (1, 2, 3):
            assert np.isnan(outs["case"][i][RC.SPECIAL_AT]), (name, i)
    rest = np.ones((2, 8), bool)
    rest[RC.SPECIAL_AT] = False
    for a, b in zip(outs["case"], outs["base"]):
        assert_bits(a[rest], b[rest], "away from the special element")
