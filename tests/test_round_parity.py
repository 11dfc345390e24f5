"""GPU: the AdaRound / BRECQ / QDrop kernels (dipoorlet_amd/csrc/round_kernels.hip through the C ABI) against the
reference-generated vectors (tests/golden/round_level.*) and against oracle/round_oracle.py on further seeds.
Tolerances: fp32 elementwise results 2e-6 relative (device expf / logf / powf are within a few ulp of the host's);
trajectories as in tests/test_round_oracle_golden.py.

Second half of the file: every kernel against the oracle on EVERY element of arrays large enough for the second trip of
its grid-stride loop (n > 2^20; 4 elements per thread for QDrop; 2^24 for the L2 loss), bit for bit wherever no
transcendental is involved (floor, the hard weight, Adam's moments and update given the device's own gradient, the L2
gradient, QDrop), the kink of the rectified sigmoid, clamp and rounding ties, NaN / ±inf one at a time (the oracle is
pinned on those rows to torch autograd), the device schedule's fields, and the host-side refusal of sizes whose 32-bit
loop index would wrap.  The sparse kernels' share is in tests/test_sparse_quant.py; shared inputs in
tests/round_cases.py."""
import ctypes as C
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


def close(a, b, rtol=2e-6, atol=1e-7):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def mask_gradient(rp, G, reg_beta=0.0):
    """dL/d(mask) for upstream dL/d(qw) = G through the fused step kernel in gradients-only mode."""
    from dipoorlet_amd import _hip
    from dipoorlet_amd.ops import _ptr, _stream
    from dipoorlet_amd.weight_transform.ada_quant_layer import _step_params
    g = torch.empty_like(rp.round_mask)
    val = torch.zeros(1, dtype=torch.float64, device="cuda")
    p = _step_params(adam=0, clamp=rp.clamp, reg_beta=reg_beta)
    _hip.check(_hip.lib().dpl_round_step(_ptr(G) if G is not None else None, _ptr(rp.wfloor), _ptr(rp.round_mask), None,
                                         None, _ptr(rp.scale), _ptr(rp.q_min), _ptr(rp.q_max), rp.n, rp.nch, rp.inner,
                                         C.byref(p), None, None, _ptr(g), _ptr(val), _stream()), "dpl_round_step")
    return g, float(val[0])


@pytest.mark.parametrize("case", META["quant_weight"], ids=lambda c: c["key"])
def test_quant_weight_golden(case):
    from dipoorlet_amd.weight_transform.ada_quant_layer import RoundingParam, quant_weight
    k = case["key"]
    w, mask, G, scale = dev(Z[k + "_w"]), dev(Z[k + "_mask"]), dev(Z[k + "_G"]), dev(Z[k + "_scale"])
    qmin, qmax = torch.full_like(scale, -127.0), torch.full_like(scale, 127.0)
    close(quant_weight(w, mask, scale, qmin, qmax, case["per_channel"], soft=True), Z[k + "_soft"])
    assert np.array_equal(quant_weight(w, mask, scale, qmin, qmax, case["per_channel"], soft=False).cpu().numpy(),
                          Z[k + "_hard"])
    rp = RoundingParam(w, scale, qmin, qmax, case["per_channel"])
    close(rp.round_mask, Z[k + "_alpha0"], rtol=1e-5, atol=2e-6)
    if not case["tight"]:     # nothing clamps: h(alpha0) gives the weight back
        close(rp.qw, Z[k + "_w"], rtol=0, atol=float(scale.max()) * 2e-6 * 127)
    rp.round_mask.copy_(mask)
    g, _ = mask_gradient(rp, G)
    close(g, Z[k + "_grad"], rtol=5e-6, atol=1e-9)


def test_regulariser_golden():
    from dipoorlet_amd.weight_transform.ada_quant_layer import TempDecay, adaround_reg
    mask = dev(Z["reg_mask"])
    close(adaround_reg().rectified_sigmoid(mask), Z["rect_sigmoid"])
    for t, v in META["temp_decay_1000"].items():
        assert TempDecay(1000)(int(t)) == pytest.approx(v, abs=1e-12)
    for row in META["reg"]:
        reg = adaround_reg(row["max_iter"])
        val, g = reg.value_and_grad(mask, row["iter"])
        assert reg.beta == pytest.approx(row["beta"], abs=1e-9)
        assert float(val) == pytest.approx(row["value"], rel=2e-5, abs=1e-6)
        close(g, Z[f"reg_grad_{row['max_iter']}_{row['iter']}"], rtol=2e-4, atol=2e-8)


def test_l2_norm_golden_and_relu():
    from dipoorlet_amd.weight_transform.ada_quant_layer import L2_norm
    from oracle import round_oracle as ro
    for row in META["l2"]:
        k = row["key"]
        val, g = L2_norm(dev(Z[k + "_pred"]), dev(Z[k + "_tgt"]))
        assert float(val) == pytest.approx(row["value"], rel=1e-6)
        close(g, Z[k + "_grad"])
    rng = np.random.default_rng(3)
    for shape in ((5, 7, 9, 11), (3, 1000), (2, 3, 5)):          # ragged sizes: the scalar tail of the vector kernel
        p, t = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
        for relu in (False, True):
            ev, eg = ro.l2_value_grad(p, t, relu)
            val, g = L2_norm(dev(p), dev(t), relu=relu)
            assert float(val) == pytest.approx(ev, rel=1e-6)
            close(g, eg)
    # accumulation into a caller buffer and a non-16-B-aligned view
    buf = torch.zeros(1, dtype=torch.float64, device="cuda")
    p = dev(rng.standard_normal(4099).astype(np.float32))[1:].reshape(2, -1)
    t = torch.zeros_like(p)
    L2_norm(p, t, loss=buf)
    L2_norm(p, t, loss=buf)
    assert float(buf) == pytest.approx(2 * float((p.double() ** 2).sum()) / 2, rel=1e-9)


def test_quant_acti_drop_golden_and_autograd():
    from dipoorlet_amd.weight_transform.ada_quant_layer import quant_acti
    d = META["drop"][0]
    x, r, G = dev(Z["drop_x"]), dev(Z["drop_r"]), dev(Z["drop_G"])
    y = quant_acti(x, d["scale"], d["q_min"], d["q_max"], d["prob"], rand=r)
    assert np.array_equal(y.cpu().numpy(), Z["drop_y"])
    # the autograd path draws its own uniform numbers: the gradient is 1 exactly where the value was kept
    xa = x.clone().requires_grad_(True)
    torch.manual_seed(0)
    ya = quant_acti(xa, d["scale"], d["q_min"], d["q_max"], 0.5)
    (ya * G).sum().backward()
    kept = (ya.detach() == x) & (ya.detach() != quant_acti(x, d["scale"], d["q_min"], d["q_max"], 1.0))
    quantised = ya.detach() != x
    assert torch.equal(xa.grad[kept], G[kept]) and float(xa.grad[quantised].abs().sum()) == 0.0
    assert 0.35 < float(quantised.float().mean()) < 0.65
    # prob = 1: everything quantised, no gradient
    xb = x.clone().requires_grad_(True)
    quant_acti(xb, d["scale"], d["q_min"], d["q_max"], 1.0).sum().backward()
    assert float(xb.grad.abs().sum()) == 0.0


def test_step_matches_oracle_on_more_seeds():
    """One fused step (gradient + regulariser + Adam + refreshed weight) against the hand-written oracle."""
    from dipoorlet_amd.weight_transform.ada_quant_layer import RoundingParam
    from oracle import round_oracle as ro
    rng = np.random.default_rng(11)
    for shape, pc in (((16, 8, 3, 3), True), ((16, 8, 3, 3), False), ((10, 33), True), ((1, 7), False)):
        w = (rng.standard_normal(shape) * 0.1).astype(np.float32)
        amax = np.abs(w).reshape(shape[0], -1).max(1) if pc else np.abs(w).max(keepdims=True).reshape(1)
        scale = (amax / 100.0).astype(np.float32)             # < 127: some channels clamp
        qmin, qmax = np.full_like(scale, -127.0), np.full_like(scale, 127.0)
        rp = RoundingParam(dev(w), dev(scale), dev(qmin), dev(qmax), pc)
        _, mask = ro.alpha_init(w, scale)
        opt = ro.Adam(mask.shape)
        for it, beta in enumerate((0.0, 20.0, 7.5)):
            G = rng.standard_normal(shape).astype(np.float32)
            _, dq = ro.quant_weight(w, mask, scale, qmin, qmax, pc)
            rv, rg = ro.reg_value_grad(mask, beta)
            mask = opt.step(mask, (G * dq).astype(np.float32) + rg)
            rp.qw.grad = dev(G)
            regbuf = torch.zeros(1, dtype=torch.float64, device="cuda")
            rp.step(beta, reg_loss=regbuf)
            assert float(regbuf) == pytest.approx(rv, rel=3e-5, abs=1e-6)
            diff = np.abs(rp.round_mask.cpu().numpy() - mask)
            assert np.mean(diff < 3e-6) > 0.995 and diff.max() <= 2.1e-3 * (it + 1), (shape, pc, it, diff.max())
            mask = rp.round_mask.cpu().numpy().copy()          # re-synchronise: compare step by step
            opt.m, opt.v = rp.exp_avg.cpu().numpy().copy(), rp.exp_avg_sq.cpu().numpy().copy()
            close(rp.qw, ro.quant_weight(w, mask, scale, qmin, qmax, pc)[0], rtol=3e-6, atol=1e-8)
        assert np.array_equal(rp.hard_weight().cpu().numpy(), ro.quant_weight(w, mask, scale, qmin, qmax, pc, soft=False)[0])


def _node(kind):
    from dipoorlet_amd.onnx_io import Node
    if kind == "gemm":
        return Node("Gemm", ["x", "w", "b"], ["y"], name="fc", attrs={"transB": 1})
    return Node("Conv", ["x", "w", "b"], ["y"], name="conv", attrs={"pads": [1, 1, 1, 1], "kernel_shape": [3, 3],
                                                                     "strides": [1, 1], "dilations": [1, 1], "group": 1})


@pytest.mark.parametrize("row", META["traj"], ids=lambda r: r["key"])
def test_training_trajectory_golden(row):
    """learning_round_mask on the GPU against the reference's CPU trajectory."""
    from dipoorlet_amd.weight_transform.ada_quant_layer import AdaQLayer, adaround_reg
    from dipoorlet_amd.weight_transform.reconstruction import learn_rounding
    k = row["key"]
    scale = dev(Z[k + "_scale"])
    qw = {"scale": scale, "q_min": torch.full_like(scale, row["q_min"]), "q_max": torch.full_like(scale, row["q_max"]),
          "per_channel": row["per_channel"], "type": "Linear"}
    layer = AdaQLayer(_node(row["kind"]), dev(Z[k + "_w"]), dev(Z[k + "_b"]), qw, None, row["relu"], False)
    snaps = {}

    def grab(it, layers):
        if it in (1, 10, row["total_iter"]):
            snaps[it] = layers[0].round_mask.cpu().numpy().copy()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    learn_rounding([layer], dev(Z[k + "_x"]), None, dev(Z[k + "_fp"]), adaround_reg(row["total_iter"]), row["bs"],
                   row["epochs"], on_step=grab)
    for step, tol in ((1, 2e-6), (10, 5e-5), (row["total_iter"], 1e-3)):
        diff = np.abs(snaps[step] - Z[f"{k}_mask_{step}"])
        assert np.mean(diff <= tol) >= 0.95, (step, float(np.mean(diff <= tol)), float(diff.max()))
        assert diff.max() <= 2.5e-3 * step
    assert np.mean(layer.new_weight().cpu().numpy() == Z[k + "_hard"]) >= 0.97
    assert layer.rp.steps == row["total_iter"]


def test_graph_replay_equals_eager():
    """The hipGraph-replayed loop and the eager loop run the same kernels: masks must agree to rounding noise of the
    library convolutions, and both must have advanced the device schedule identically."""
    from dipoorlet_amd.weight_transform.ada_quant_layer import AdaQLayer, adaround_reg
    from dipoorlet_amd.weight_transform.reconstruction import learn_rounding
    row = next(r for r in META["traj"] if r["kind"] == "conv")
    k = row["key"]
    res = {}
    for mode in (False, True):
        scale = dev(Z[k + "_scale"])
        qw = {"scale": scale, "q_min": torch.full_like(scale, row["q_min"]), "q_max": torch.full_like(scale, row["q_max"]),
              "per_channel": row["per_channel"], "type": "Linear"}
        layer = AdaQLayer(_node("conv"), dev(Z[k + "_w"]), dev(Z[k + "_b"]), qw, None, row["relu"], False)
        reg = adaround_reg(row["total_iter"])
        learn_rounding([layer], dev(Z[k + "_x"]), None, dev(Z[k + "_fp"]), reg, row["bs"], row["epochs"], use_graph=mode)
        res[mode] = (layer.round_mask.cpu().numpy().copy(), reg.beta, layer.rp.steps)
    assert res[True][1] == res[False][1] and res[True][2] == res[False][2] == row["total_iter"]
    diff = np.abs(res[True][0] - res[False][0])
    assert np.mean(diff <= 1e-5) >= 0.99 and diff.max() <= 2.5e-3 * row["total_iter"]
    assert np.mean(np.abs(res[True][0] - Z[f"{k}_mask_{row['total_iter']}"]) <= 1e-3) >= 0.95


# ====================================================================================================================
# The ten kernels through the C ABI against oracle/round_oracle.py, at sizes that take every grid-stride loop round a
# second time, bit for bit wherever no transcendental is involved, and at constructed edges.  Host inputs are generated
# once per process (round_cases.layout_data, _l2_host).
import round_cases as RC                                   # noqa: E402
from round_cases import assert_bits, assert_close_specials  # noqa: E402

F32 = np.float32


def _lib():
    from dipoorlet_amd import _hip
    return _hip.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ok(status, what):
    from dipoorlet_amd import _hip
    _hip.check(status, what)


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


def k_init(d):
    n, nch, inner = _chan(d)
    sc, lo, hi = _grid(d)
    w = dev(d["w"])
    wf, a = torch.empty_like(w), torch.empty_like(w)
    _ok(_lib().dpl_round_init(_p(w), _p(sc), n, nch, inner, _p(wf), _p(a), None), "dpl_round_init")
    return wf, a


def k_quant(d, wfloor, mask, soft, clamp=None):
    n, nch, inner = _chan(d)
    sc, lo, hi = _grid(d)
    out = torch.empty_like(wfloor)
    _ok(_lib().dpl_round_quant(_p(wfloor), _p(mask), _p(sc), _p(lo), _p(hi), n, nch,
                               inner, int(d["pc"] if clamp is None else clamp), soft, _p(out), None), "dpl_round_quant")
    return out


def k_step(d, G, wfloor, alpha, m=None, v=None, step=1, adam=0, beta=0.0, lam=0.01, grad_scale=1.0, sched=None,
           want_qw=False, reg=None, want_g=True):
    """dpl_round_step on device tensors (alpha, m, v updated in place when adam) -> (g, qw_next)."""
    from dipoorlet_amd.weight_transform.ada_quant_layer import _step_params
    n, nch, inner = _chan(d)
    sc, lo, hi = _grid(d)
    p = _step_params(step=step, adam=adam, clamp=int(d["pc"]), grad_scale=grad_scale, reg_beta=beta, reg_lambda=lam)
    g = torch.full_like(wfloor, 777.0) if want_g else None
    qw = torch.full_like(wfloor, 777.0) if want_qw else None
    _ok(_lib().dpl_round_step(_p(G), _p(wfloor), _p(alpha), _p(m), _p(v), _p(sc), _p(lo),
                              _p(hi), n, nch, inner, C.byref(p), _p(sched), _p(qw), _p(g), _p(reg), None),
        "dpl_round_step")
    return g, qw


def oracle_grad_parts(d, mask, G, beta, lam=0.01, grad_scale=1.0, inside=None):
    """(quantiser part, regulariser part of dL/d(mask), regulariser value) as autograd gives them for upstream G * grad_scale."""
    from oracle import round_oracle as ro
    _, dq = ro.quant_weight(d["w"], mask, d["scale"], d["qmin"], d["qmax"], d["pc"], inside=inside)
    rv, rg = ro.reg_value_grad(mask, beta, lam, inside=inside)
    with np.errstate(invalid="ignore"):
        return ((G * F32(grad_scale)).astype(F32) * dq).astype(F32), rg, rv


def oracle_grad(d, mask, G, beta, lam=0.01, grad_scale=1.0, inside=None):
    gq, rg, rv = oracle_grad_parts(d, mask, G, beta, lam, grad_scale, inside)
    with np.errstate(invalid="ignore"):
        return gq + rg, rv


def _grad_close(got, gq, rg, what):
    """|got - (gq + rg)| <= 5e-6 |gq| + 2e-4 |rg| + 2e-8, NaN / ±inf in the same places: each part at the bound the golden
    tests put on it — 5e-6 on the gradient through the quantiser (test_quant_weight_golden), 2e-4 and 2e-8 on the
    regulariser's (test_regulariser_golden: u^(beta-1) magnifies the last bits of h by beta - 1).  Measured on MI355X: the
    quantiser part alone (beta = 0) is within 5e-6; the worst deviation with the regulariser on is 2.9e-7 absolute, about
    8e-6 of that part (|rg| = 0.037 there), at beta = 20 on masks one Adam step inside the kink (u = 1 - 1.8e-4)."""
    with np.errstate(invalid="ignore"):
        want = (gq + rg).astype(np.float64)
    got = np.asarray(got, np.float64)
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(got), f(want)), (what, f.__name__, np.argwhere(f(got) != f(want))[:4].tolist())
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    bound = 5e-6 * np.abs(gq[fin].astype(np.float64)) + 2e-4 * np.abs(rg[fin].astype(np.float64)) + 2e-8
    assert np.all(err <= bound), (what, int((err > bound).sum()), float(err.max()), float((err / bound).max()))


def check_grad(d, mask, G, beta, got, grad_scale=1.0, what=""):
    """The mask gradient against the oracle at _grad_close's bounds.  On the kink (round_cases.kink) g is either branch:
    exactly zero, or the value with dh passed."""
    gq, rg, rv = oracle_grad_parts(d, mask, G, beta, grad_scale=grad_scale)
    kink = RC.kink(mask)
    assert kink.mean() <= 0.002, (what, float(kink.mean()))
    _grad_close(got[~kink], gq[~kink], rg[~kink], what)
    if kink.any():
        iq, ir, _ = oracle_grad_parts(d, mask, G, beta, grad_scale=grad_scale, inside=np.ones(mask.shape, bool))
        gk = got[kink].astype(np.float64)
        ik = (iq[kink] + ir[kink]).astype(np.float64)
        bound = 5e-6 * np.abs(iq[kink].astype(np.float64)) + 2e-4 * np.abs(ir[kink].astype(np.float64)) + 2e-8
        assert np.all((gk == 0) | (np.abs(gk - ik) <= bound)), what
    return rv, int(kink.sum())


@pytest.mark.parametrize("name", [r[0] for r in RC.LAYOUTS])
def test_round_init_and_quant_second_trip(name):
    """dpl_round_init and dpl_round_quant (soft, hard) on every element of arrays with n > 2^20 (and 2^20 - 1, 2^20): wfloor
    and the hard weight bit for bit, the initial mask and the soft weight at the bounds of test_quant_weight_golden."""
    from oracle import round_oracle as ro
    d = RC.layout_data(name)
    wf, a0 = k_init(d)
    assert_bits(host(wf), d["wfloor"], "wfloor")
    close(a0, d["alpha0"], rtol=1e-5, atol=2e-6)
    for mask in (d["alpha0"], d["trained"]):
        soft = host(k_quant(d, wf, dev(mask), 1))
        close(soft, ro.quant_weight(d["w"], mask, d["scale"], d["qmin"], d["qmax"], d["pc"])[0])
        hard = host(k_quant(d, wf, dev(mask), 0))
        assert_bits(hard, ro.quant_weight(d["w"], mask, d["scale"], d["qmin"], d["qmax"], d["pc"], soft=False)[0], "hard")
    if d["pc"] and d["shape"][-1] != 1:
        assert (np.abs(soft / ro._bc(d["scale"], soft.ndim)) == 127).any()             # the clamp was exercised


@pytest.mark.parametrize("name", [r[0] for r in RC.LAYOUTS])
def test_round_step_gradients_second_trip_and_kink(name):
    """dpl_round_step in gradients-only mode on the large layouts, at the initial mask (every exact multiple of the scale sits
    on the kink: all zero weights) and at a trained one, for beta 0 / 20 / 7.5; alpha, and absent moments, stay untouched."""
    d = RC.layout_data(name)
    wf = dev(d["wfloor"])
    kinks = []
    for mask, G, beta in ((d["alpha0"], d["G"], 0.0), (d["alpha0"], d["G2"], 20.0), (d["trained"], d["G3"], 7.5),
                          (d["trained"], None, 2.0)):
        a = dev(mask)
        reg = torch.full((1,), 5.0, dtype=torch.float64, device="cuda")
        g, _ = k_step(d, None if G is None else dev(G), wf, a, beta=beta, reg=reg)
        rv, nk = check_grad(d, mask, np.zeros_like(mask) if G is None else G, beta, host(g), what=(name, beta))
        kinks.append(nk)
        assert float(reg) - 5.0 == pytest.approx(rv, rel=3e-5, abs=1e-6)
        assert beta > 0 or float(reg) == 5.0
        assert_bits(host(a), mask, "alpha untouched")
    assert kinks[0] >= d["w"].size // 2000 and kinks[0] == kinks[1]      # the zero weights ARE on the kink


@pytest.mark.parametrize("grad_scale", (1.0, 0.5))
@pytest.mark.parametrize("name", [r[0] for r in RC.LAYOUTS])
def test_adam_step_exact_given_the_devices_gradient(name, grad_scale):
    """Three consecutive full steps (beta 0, 20, 7.5).  The kernel hands out the very g it feeds to Adam (d_grad_alpha), so
    with that g the oracle's Adam must reproduce m and v bit for bit (fp32 multiplies and adds, no contraction) and alpha too
    (sqrtf and the divides are correctly rounded under the build's default -fhip-fp32-correctly-rounded-divide-sqrt).
    g itself is held to the oracle at check_grad's bounds, the refreshed weight to the oracle at the device's new alpha."""
    from oracle import round_oracle as ro
    d = RC.layout_data(name)
    wf = dev(d["wfloor"])
    mask = d["alpha0"].copy()
    a, m, v = dev(mask), torch.zeros_like(wf), torch.zeros_like(wf)
    opt = ro.Adam(mask.shape)
    for it, (beta, G) in enumerate(((0.0, d["G"]), (20.0, d["G2"]), (7.5, d["G3"]))):
        reg = torch.zeros(1, dtype=torch.float64, device="cuda")
        g, qw = k_step(d, dev(G), wf, a, m, v, step=it + 1, adam=1, beta=beta, grad_scale=grad_scale, want_qw=True, reg=reg)
        g = host(g)
        rv, _ = check_grad(d, mask, G, beta, g, grad_scale, what=(name, it))
        assert float(reg) == pytest.approx(rv, rel=3e-5, abs=1e-6)
        want_alpha = opt.step(mask, g)
        assert_bits(host(m), opt.m, f"exp_avg step {it + 1}")
        assert_bits(host(v), opt.v, f"exp_avg_sq step {it + 1}")
        mask = host(a).copy()
        print(f"{name} gs={grad_scale} step {it + 1}: alpha worst ulp distance {int(RC.ulp_distance(mask, want_alpha).max())}")
        assert_bits(mask, want_alpha, f"alpha step {it + 1}")
        close(qw, ro.quant_weight(d["w"], mask, d["scale"], d["qmin"], d["qmax"], d["pc"])[0], rtol=3e-6, atol=1e-8)
        assert np.abs(mask - d["alpha0"]).max() <= 1.01e-3 * (it + 1)       # Adam moves at most lr per step


# ---- constructed edges: power-of-two scales, so that w = k * scale is exact
def _edge(w, scale, qmin, qmax, pc=True):
    w = np.asarray(w, F32)
    return {"w": w, "scale": np.asarray(scale, F32).reshape(-1), "qmin": np.asarray(qmin, F32).reshape(-1),
            "qmax": np.asarray(qmax, F32).reshape(-1), "pc": pc, "shape": w.shape}


def test_clamp_ties_split_the_gradient_in_half():
    """wfloor + h exactly on q_max / q_min, just inside and just outside.  A saturated mask gives h = 0 or 1 exactly (and
    dh = 0: the value is checked); to SEE the factor the grid is moved by a half, so that mask = 0 (h = 0.5 exactly,
    dh = 0.3) lands on the bound: the factor is 1 inside, 0.5 on the tie, 0 outside and never 0.25."""
    from oracle import round_oracle as ro
    s = F32(2.0 ** -7)
    k = np.array([126, 127, 127, 125, -127, -128, -128, -126, 128, -129], F32)
    big = np.array([1e30, -1e30, 1e30, 1e30, -1e30, 1e30, -1e30, -1e30, -1e30, 1e30], F32)
    d = _edge(k * s, [s], [-127], [127])
    wf, _ = k_init(d)
    assert_bits(host(wf), k, "floor of exact multiples")
    qw = host(k_quant(d, wf, dev(big), 1))
    assert_bits(qw, np.array([127, 127, 127, 126, -127, -127, -127, -126, 127, -127], F32) * s, "saturated")
    assert_bits(qw, ro.quant_weight(d["w"], big, d["scale"], d["qmin"], d["qmax"], True)[0], "saturated / oracle")
    # half-integer bounds: floor + 0.5 against [-126.5, 126.5]
    k2 = np.array([126, 125, 127, -127, -126, -128, 0, 126, -127], F32)
    d2 = _edge(k2 * s, [s], [-126.5], [126.5])
    G = np.array([1, 2, 3, 4, 5, 6, 7, -8, -9], F32)
    zero = np.zeros(9, F32)
    g, _ = k_step(d2, dev(G), dev(k2), dev(zero))
    factor = host(g) / (G * s * F32(0.3))
    np.testing.assert_allclose(factor, [0.5, 1, 0, 0.5, 1, 0, 1, 0.5, 0.5], rtol=1e-6, atol=0)
    assert_close_specials(host(g), oracle_grad(d2, zero, G, 0.0)[0], 5e-6, 0)
    qw2 = host(k_quant(d2, dev(k2), dev(zero), 1))
    assert_bits(qw2, np.array([126.5, 125.5, 126.5, -126.5, -125.5, -126.5, 0.5, 126.5, -126.5], F32) * s, "half grid")
    # one ulp inside / outside the bound: q_max = nextafter(126.5, ±inf)
    for qmax, f in ((np.nextafter(F32(126.5), F32(200)), 1.0), (np.nextafter(F32(126.5), F32(0)), 0.0)):
        d3 = _edge(k2[:1] * s, [s], [-127], [qmax])
        g3, _ = k_step(d3, dev(G[:1]), dev(k2[:1]), dev(zero[:1]))
        assert float(host(g3)[0]) == pytest.approx(f * float(G[0] * s * F32(0.3)), rel=1e-6, abs=0)


_MASKS = np.array([0.0, -0.0, 2.3978953, -2.3978953, 88.8, -88.8, 104, -104, 1e30, -1e30, np.inf, -np.inf]
                  + [np.nextafter(F32(sg * 2.3978953), F32(to)) for sg in (1, -1) for to in (9, -9)], F32)


def test_mask_edges_soft_hard_and_gradient():
    """Masks at zero of either sign, at the kink (±ln 11 and its fp32 neighbours), where expf overflows (|a| > 88.7) or the
    sigmoid saturates, and at ±inf.  The hard weight takes mask = -0.0 as >= 0."""
    from oracle import round_oracle as ro
    s = F32(2.0 ** -5)
    k = np.arange(len(_MASKS), dtype=F32) - 8
    d = _edge(k * s, [s], [-127], [127])
    G = (np.arange(len(_MASKS), dtype=F32) + 1) / 4
    wf = dev(k)
    assert_close_specials(host(k_quant(d, wf, dev(_MASKS), 1)), ro.quant_weight(d["w"], _MASKS, [s], [-127], [127], True)[0],
                          2e-6, 1e-7)
    hard = host(k_quant(d, wf, dev(_MASKS), 0))
    assert_bits(hard, ro.quant_weight(d["w"], _MASKS, [s], [-127], [127], True, soft=False)[0], "hard")
    assert hard[1] == (k[1] + 1) * s and hard[3] == k[3] * s                 # -0.0 -> ceil, -2.39 -> floor
    for beta in (0.0, 2.0, 20.0):
        reg = torch.zeros(1, dtype=torch.float64, device="cuda")
        g, _ = k_step(d, dev(G), wf, dev(_MASKS), beta=beta, reg=reg)
        want, rv = oracle_grad(d, _MASKS, G, beta)
        kink = RC.kink(_MASKS)
        assert kink.sum() == 6                                                 # ±ln 11 and both neighbours of each
        assert_close_specials(host(g)[~kink], want[~kink], 5e-6, 2e-8, beta)
        g_in, _ = oracle_grad(d, _MASKS, G, beta, inside=np.ones(_MASKS.shape, bool))
        gk = host(g)[kink]
        assert np.all((gk == 0) | (np.abs(gk - g_in[kink]) <= 5e-6 * np.abs(g_in[kink]) + 2e-8))
        assert float(reg) == pytest.approx(rv, rel=3e-5, abs=1e-6)
        assert np.all(host(g)[4:12] == 0)                                      # saturated: no gradient of either kind


def test_regulariser_at_h_half_and_beta_zero():
    """mask = 0: h = 0.5 exactly, u = |h - 0.5| * 2 = 0 and sign(0) = 0.  beta = 2: value lambda per element, gradient
    exactly zero (2 * u^1 = 0).  beta = 0: value and gradient exactly zero and *reg_loss is not touched at all."""
    d = _edge(np.zeros(300, F32), [1.0], [-127], [127], pc=False)
    zero = dev(np.zeros(300, F32))
    for beta, want in ((2.0, 300 * 0.01), (20.0, 300 * 0.01)):
        reg = torch.zeros(1, dtype=torch.float64, device="cuda")
        g, _ = k_step(d, None, zero, zero, beta=beta, reg=reg)
        assert float(reg) == pytest.approx(want, rel=1e-7) and np.all(host(g) == 0)
    reg = torch.full((1,), 123.25, dtype=torch.float64, device="cuda")
    trained = dev(np.linspace(-6, 6, 300).astype(F32))
    g, _ = k_step(d, None, zero, trained, beta=0.0, reg=reg)
    assert float(reg) == 123.25 and np.all(host(g).view(np.uint32) == 0)


@pytest.mark.parametrize("name,d", RC.special_cases(("w", "mask", "G")), ids=lambda v: v if isinstance(v, str) else "")
def test_round_kernels_keep_a_special_value_in_its_element(name, d):
    """One NaN / +inf / -inf in the weight, the mask or the upstream gradient: every output has NaN / ±inf exactly where the
    oracle (pinned to torch autograd on these rows: test_round_oracle_golden.py) has them, the regulariser scalar is NaN
    exactly when the oracle's is, and no other element differs from the run without the special value."""
    from oracle import round_oracle as ro
    d = dict(d, pc=True, shape=d["w"].shape)
    base = dict(RC.special_base(), pc=True)
    outs = {}
    for key, c in (("case", d), ("base", base)):
        wf, a0 = k_init(c)
        mask = dev(c["mask"])
        soft, hard = k_quant(c, wf, mask, 1), k_quant(c, wf, mask, 0)
        reg = torch.zeros(1, dtype=torch.float64, device="cuda")
        m, v = torch.zeros_like(wf), torch.zeros_like(wf)
        g, qw = k_step(c, dev(c["G"]), wf, mask, m, v, adam=1, beta=20.0, want_qw=True, reg=reg)
        outs[key] = [host(t) for t in (wf, a0, soft, hard, g, m, v, mask, qw)] + [float(reg)]
    got = outs["case"]
    owf, oa0 = ro.alpha_init(d["w"], d["scale"])
    assert_bits(got[0], owf, "wfloor")
    assert_close_specials(got[1], oa0, 1e-5, 2e-6, "alpha0")
    assert_close_specials(got[2], ro.quant_weight(d["w"], d["mask"], d["scale"], d["qmin"], d["qmax"], True)[0], 2e-6, 1e-7)
    assert_bits(got[3], ro.quant_weight(d["w"], d["mask"], d["scale"], d["qmin"], d["qmax"], True, soft=False)[0], "hard")
    og, rv = oracle_grad(d, d["mask"], d["G"], 20.0)
    assert_close_specials(got[4], og, 5e-6, 2e-8, "g")
    assert np.isnan(got[9]) == np.isnan(rv) and (np.isnan(rv) or got[9] == pytest.approx(rv, rel=3e-5, abs=1e-6))
    opt = ro.Adam(d["mask"].shape)
    with np.errstate(invalid="ignore"):
        want_alpha = opt.step(d["mask"], got[4])
    assert_bits(got[5], opt.m, "m")
    assert_bits(got[6], opt.v, "v")
    assert_bits(got[7], want_alpha, "alpha")
    if name.endswith("nan"):
        for i in (4, 5, 6, 7, 8) if not name.startswith("w") else (0, 1, 2, 3, 8):
            assert np.isnan(got[i][RC.SPECIAL_AT]), (name, i)
    rest = np.ones(d["w"].shape, bool)
    rest[RC.SPECIAL_AT] = False
    for i in range(9):
        assert_bits(got[i][rest], outs["base"][i][rest], f"output {i} away from the special element")


# ---- L2 loss: the vector kernel's unrolled body takes its second trip for n > 2^24, the scalar kernel likewise
_L2_N = 32 * 256 * 56 * 56
_L2 = {}


def _l2_host():
    if not _L2:
        rng = np.random.default_rng(2024)
        _L2["z"] = rng.standard_normal(_L2_N + 8, dtype=F32)
        _L2["t"] = rng.standard_normal(_L2_N + 8, dtype=F32)
    return _L2["z"], _L2["t"]


def _l2_oracle(z, t, relu, m):
    y = np.where(z < 0, F32(0), z) if relu else z
    dd = (y - t).astype(F32)
    g = (F32(F32(1.0 / m) * F32(2)) * dd).astype(F32)
    return float(np.sum((dd * dd).astype(np.float64))) / m, (np.where(z <= 0, F32(0), g).astype(F32) if relu else g)


def _l2_run(zb, tb, gb, off, n, relu, m, loss):
    """dpl_l2_loss on the n elements `off` (z, t, grad: one each) elements into device buffers -> the gradient, and whether
    the gradient buffer is untouched before and behind those n."""
    ptr = [C.c_void_p(b.data_ptr() + 4 * o) for b, o in zip((zb, tb, gb), off)]
    gb.fill_(777.0)
    _ok(_lib().dpl_l2_loss(ptr[0], ptr[1], n, relu, float(F32(1.0 / m) * F32(2)), 1.0 / m, ptr[2], _p(loss), None),
        "dpl_l2_loss")
    return host(gb[off[2]:off[2] + n]), bool((gb[:off[2]] == 777.0).all()) and bool((gb[off[2] + n:] == 777.0).all())


def test_l2_oracle_restates_round_oracle():
    from oracle import round_oracle as ro
    rng = np.random.default_rng(8)
    z, t = rng.standard_normal((6, 5, 7)).astype(F32), rng.standard_normal((6, 5, 7)).astype(F32)
    for relu in (False, True):
        v0, g0 = ro.l2_value_grad(z, t, relu)
        v1, g1 = _l2_oracle(z.reshape(-1), t.reshape(-1), relu, 42)
        assert v0 == v1 and np.array_equal(g0.reshape(-1), g1)


@pytest.mark.parametrize("relu", (0, 1))
def test_l2_loss_vector_kernel_second_trip(relu):
    """k_l2_loss<true> at n around 2^24 (one lane's four unrolled vectors end / start a second trip there), with n mod 4 =
    1, 2, 3 behind it, and at a batch-32 layer1 activation.  The gradient of EVERY element bit for bit; the loss (an fp64 sum
    of fp32 squares: summation order only) to 1e-9 relative, fresh and accumulated onto a previous value; nothing is written
    past n."""
    z, t = _l2_host()
    zb, tb = dev(z), dev(t)
    gb = torch.empty_like(zb)
    for n in (2 ** 24 - 4, 2 ** 24, 2 ** 24 + 4, 2 ** 24 + 5, 2 ** 24 + 6, 2 ** 24 + 7, _L2_N):
        m = n // 256 if n == _L2_N else 32
        want, wg = _l2_oracle(z[:n], t[:n], relu, m)
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        g, untouched = _l2_run(zb, tb, gb, (0, 0, 0), n, relu, m, loss)
        assert_bits(g, wg, f"grad n={n}")
        assert untouched
        assert float(loss) == pytest.approx(want, rel=1e-9)
        loss.fill_(-0.5 * want)          # accumulated: -want / 2 + want, each term to 1e-9 of `want` = 4e-9 of the result
        _ok(_lib().dpl_l2_loss(_p(zb), _p(tb), n, relu, 1.0, 1.0 / m, None, _p(loss), None), "dpl_l2_loss")   # no gradient wanted
        assert float(loss) == pytest.approx(0.5 * want, rel=4e-9)


@pytest.mark.parametrize("relu", (0, 1))
def test_l2_loss_scalar_kernel_each_operand_off_16_bytes(relu):
    """k_l2_loss<false>: z, the target or the gradient (one at a time) one element into its buffer, at 25 690 112 elements
    (the scalar loop's second trip starts at 2^23) and at 1001."""
    z, t = _l2_host()
    zb, tb = dev(z), dev(t)
    gb = torch.empty_like(zb)
    for n in (_L2_N, 1001):
        for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            want, wg = _l2_oracle(z[off[0]:off[0] + n], t[off[1]:off[1] + n], relu, 32)
            loss = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")
            g, untouched = _l2_run(zb, tb, gb, off, n, relu, 32, loss)
            assert_bits(g, wg, f"grad n={n} off={off}")
            assert untouched
            assert float(loss) - 3.0 == pytest.approx(want, rel=1e-9)


@pytest.mark.parametrize("name,d", RC.special_cases(("z", "t")), ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("relu", (0, 1))
def test_l2_loss_special_values(name, d, relu):
    """One NaN / ±inf in the pre-activation or the target, on either side of the ReLU, on both kernels: the gradient bit for
    bit as autograd gives it (a NaN pre-activation has a NaN gradient, ReLU or not; a NaN target behind a closed ReLU has
    gradient 0), the loss NaN / inf as the oracle's, every other gradient element as without the special value."""
    from dipoorlet_amd.weight_transform.ada_quant_layer import L2_norm
    from oracle import round_oracle as ro
    for sign in (1, -1):
        zz = d["z"].copy()
        if np.isfinite(zz[RC.SPECIAL_AT]):
            zz[RC.SPECIAL_AT] = sign * abs(zz[RC.SPECIAL_AT])
        want, wg = ro.l2_value_grad(zz, d["t"], bool(relu))
        for view in (False, True):                    # aligned (vector kernel) and one element in (scalar kernel)
            zt, tt = dev(zz), dev(d["t"])
            if view:
                zt = torch.cat([zt.new_zeros(1), zt.reshape(-1)])[1:].reshape(zz.shape)
            val, g = L2_norm(zt, tt, relu=bool(relu))
            assert_bits(host(g), wg, (name, sign, view))
            val = float(val)
            assert (np.isnan(want) and np.isnan(val)) or val == pytest.approx(want, rel=1e-6), (name, want, val)
        if name == "z=nan" or name == "z=+inf" or (name == "z=-inf" and not relu):
            assert not np.isfinite(val) and not np.isfinite(wg[RC.SPECIAL_AT])
        b = RC.special_base()
        b["z"][RC.SPECIAL_AT] = zz[RC.SPECIAL_AT] if np.isfinite(zz[RC.SPECIAL_AT]) else b["z"][RC.SPECIAL_AT]
        rest = np.ones(zz.shape, bool)
        rest[RC.SPECIAL_AT] = False
        assert_bits(host(g)[rest], ro.l2_value_grad(b["z"], b["t"], bool(relu))[1][rest], "rest")


# ---- QDrop
def _drop(x, r, n, scale, qmin, qmax, prob, G):
    y, gx = torch.full_like(x, 777.0), torch.full_like(x, 777.0)
    _ok(_lib().dpl_acti_drop_fwd(_p(x), _p(r), n, scale, qmin, qmax, prob, _p(y), None), "dpl_acti_drop_fwd")
    _ok(_lib().dpl_acti_drop_bwd(_p(r), _p(G), n, prob, _p(gx), None), "dpl_acti_drop_bwd")
    return host(y), host(gx)


def test_acti_drop_second_trip():
    """dpl_acti_drop_fwd / _bwd past 4 elements per thread of the capped grid (n > 4 194 304), every element bit for bit."""
    from oracle import round_oracle as ro
    rng = np.random.default_rng(31)
    nmax = 6422528                                          # (32, 64, 56, 56)
    x, r, G = (rng.standard_normal(nmax, dtype=F32) * 3), rng.random(nmax, dtype=F32), rng.standard_normal(nmax, dtype=F32)
    xb, rb, Gb = dev(x), dev(r), dev(G)
    for n in (4194303, 4194305, nmax):
        y, gx = _drop(xb, rb, n, 0.0625, -128.0, 127.0, 0.5, Gb)
        oy, dy = ro.quant_acti_drop(x[:n], r[:n], 0.0625, -128.0, 127.0, 0.5)
        assert_bits(y[:n], oy, f"y n={n}")
        assert_bits(gx[:n], dy * G[:n], f"gx n={n}")
        assert np.all(y[n:] == 777.0) and np.all(gx[n:] == 777.0)
        assert 0.49 < (oy != x[:n]).mean() < 0.51 and (oy == F32(127 * 0.0625)).any() and (oy == F32(-8)).any()


def test_acti_drop_edges():
    """rint ties (half to even), -0.0, denormals, the clamp; r == prob exactly and one ulp either side (the comparison is
    r < prob); prob 0, 1 and above 1; no draw at all (everything quantised)."""
    from oracle import round_oracle as ro
    s = 0.25
    x = np.array([0.125, -0.125, 0.375, -0.375, 0.625, -0.625, -0.0, 0.0, 1e-40, -1e-40, 1.75, 1.875, 2.0, -2.0, -2.125,
                  -2.25, 100.0, -100.0, 0.126, 0.3], F32)
    n = len(x)
    G = np.arange(1, n + 1, dtype=F32)
    y, _ = _drop(dev(x), None, n, s, -8.0, 7.0, 0.5, dev(G))
    assert_bits(y, np.array([0, 0, 0.5, -0.5, 0.5, -0.5, 0, 0, 0, 0, 1.75, 1.75, 1.75, -2, -2, -2, 1.75, -2, 0.25, 0.25], F32),
                "ties")
    p = F32(0.3)
    for prob in (p, F32(0.0), F32(1.0), F32(1.5)):
        r = np.resize(np.array([prob, np.nextafter(prob, F32(-1)), np.nextafter(prob, F32(2)), 0.0, 0.999], F32), n)
        r = np.minimum(r, np.nextafter(F32(1), F32(0)))                     # a uniform draw is < 1
        for rr in (r, None):
            y, gx = _drop(dev(x), None if rr is None else dev(rr), n, s, -8.0, 7.0, float(prob), dev(G))
            oy, dy = ro.quant_acti_drop(x, rr, s, -8.0, 7.0, float(prob))
            assert_bits(y, oy, f"y prob={prob}")
            assert_bits(gx, dy * G, f"gx prob={prob}")
        if prob == p:
            y, gx = _drop(dev(x), dev(r), n, s, -8.0, 7.0, float(prob), dev(G))
            assert gx[0] == G[0] and gx[1] == 0 and gx[2] == G[2]           # r == prob keeps the value: r < prob is strict


@pytest.mark.parametrize("name,d", RC.special_cases(("x", "r")), ids=lambda v: v if isinstance(v, str) else "")
def test_acti_drop_special_values(name, d):
    """A NaN activation is NaN on either branch (torch.max / torch.min hand it on), ±inf clamps on the quantised branch; a NaN
    draw compares false and keeps the value.  Every other element as without the special value."""
    from oracle import round_oracle as ro
    base = RC.special_base()
    rest = np.ones(d["x"].shape, bool)
    rest[RC.SPECIAL_AT] = False
    for prob, r in ((0.5, d["r"]), (0.999, d["r"]), (0.5, None)):
        y, gx = _drop(dev(d["x"]), None if r is None else dev(r), d["x"].size, 0.25, -8.0, 7.0, prob, dev(d["G"]))
        oy, dy = ro.quant_acti_drop(d["x"], r, 0.25, -8.0, 7.0, prob)
        assert_bits(y.reshape(oy.shape), oy, (name, prob))
        assert_bits(gx.reshape(oy.shape), dy * d["G"], (name, prob))
        if name == "x=nan":
            assert np.isnan(y.reshape(oy.shape)[RC.SPECIAL_AT])
        by = ro.quant_acti_drop(base["x"], None if r is None else base["r"], 0.25, -8.0, 7.0, prob)[0]
        assert_bits(y.reshape(oy.shape)[rest], by[rest], "rest")


# ---- the device schedule
@pytest.mark.parametrize("t_max", (1, 7, 60, 1000, 20000))
def test_device_schedule_fields(t_max):
    """dpl_round_sched_advance t_max + 3 times from zero: the counters exact, reg_beta / step_size / bc2_sqrt within ONE fp32
    ulp of oracle.sched_fields after every advance.  Basis: both sides evaluate the same double expressions; device cos, pow
    and sqrt are within a few double ulps of the host's, which moves the fp32 cast only when the double lies within that of
    a rounding boundary, and then by one step.  The temperature switches on at the first t >= 0.2 * t_max."""
    from oracle import round_oracle as ro
    buf = torch.zeros(6, dtype=torch.int32, device="cuda")
    hist = torch.zeros(t_max + 3, 6, dtype=torch.int32, device="cuda")
    for i in range(t_max + 3):
        _ok(_lib().dpl_round_sched_advance(_p(buf), t_max, 1e-3, 0.9, 0.999, None), "dpl_round_sched_advance")
        hist[i].copy_(buf)
    h = hist.cpu().numpy()
    assert np.array_equal(h[:, 0], np.arange(1, t_max + 4)) and np.array_equal(h[:, 1], np.arange(1, t_max + 4))
    assert np.all(h[:, 5] == 0)
    got = h[:, 2:5].copy().view(F32)
    want = np.array([ro.sched_fields(t, t + 1, t_max) for t in range(t_max + 3)], F32)
    worst = RC.ulp_distance(got, want).max(0)
    print(f"t_max={t_max}: worst ulp distance (reg_beta, step_size, bc2_sqrt) = {worst.tolist()}")
    assert np.all(worst <= 1)
    first_on = next(t for t in range(t_max + 3) if not t < 0.2 * t_max)
    assert np.all(got[:first_on, 0] == 0) and np.all(got[first_on:, 0] >= 2.0) and np.all(got[first_on:, 0] <= 20.0)
    assert got[min(t_max, t_max + 2), 0] == 2.0


def test_step_with_device_schedule_equals_host_parameters():
    """One dpl_round_step reading (temperature, step size, bias correction) from a dpl_round_sched against one given the same
    iteration's host parameters: every output bit-identical.  The iteration is one where the device's three floats equal the
    host's bit for bit (they may differ by an ulp elsewhere: test_device_schedule_fields)."""
    from oracle import round_oracle as ro
    d = RC.layout_data("pc_257x4099")
    t_max = 60
    buf = torch.zeros(6, dtype=torch.int32, device="cuda")
    for it in range(1, 41):
        _ok(_lib().dpl_round_sched_advance(_p(buf), t_max, 1e-3, 0.9, 0.999, None), "dpl_round_sched_advance")
        f = buf.cpu().numpy()[2:5].copy().view(F32)
        if it >= 20 and np.array_equal(f, np.array(ro.sched_fields(it - 1, it, t_max), F32)):
            break
    else:
        raise AssertionError("no iteration in 20 .. 40 with identical fields")
    rng = np.random.default_rng(4)
    m0, v0 = (rng.standard_normal(d["w"].shape).astype(F32) * F32(1e-3)), (rng.random(d["w"].shape).astype(F32) * F32(1e-6))
    outs = []
    for sched in (buf, None):
        a, m, v = dev(d["trained"]), dev(m0), dev(v0)
        reg = torch.zeros(1, dtype=torch.float64, device="cuda")
        g, qw = k_step(d, dev(d["G"]), dev(d["wfloor"]), a, m, v, step=it if sched is None else 12345, adam=1,
                       beta=float(f[0]) if sched is None else 0.0, sched=sched, want_qw=True, reg=reg)
        outs.append([host(x) for x in (g, qw, a, m, v)] + [float(reg)])
    for x, y in zip(outs[0][:5], outs[1][:5]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert outs[0][5] == pytest.approx(outs[1][5], rel=1e-12) and outs[0][5] > 0     # atomically merged fp64 partial sums
    assert not np.array_equal(outs[0][2], d["trained"])


def test_sizes_whose_loop_index_would_wrap_are_refused():
    """The round / sparse kernels index in 32 bits with a stride of up to 2^20: n > 2^32 - 2^20 is refused on the host (-2 and a
    message) before anything is launched — null pointers are enough to see that.  Small n is accepted as before."""
    L = _lib()
    from dipoorlet_amd.weight_transform.ada_quant_layer import _step_params
    p = _step_params()
    for n in (2 ** 32 - 2 ** 20 + 1, 2 ** 32 - 1, 2 ** 32, 0, -1):
        calls = (("dpl_round_init", L.dpl_round_init(None, None, n, 1, n, None, None, None)),
                 ("dpl_round_quant", L.dpl_round_quant(None, None, None, None, None, n, 1, n, 0, 1, None, None)),
                 ("dpl_round_step", L.dpl_round_step(None, None, None, None, None, None, None, None, n, 1, n, C.byref(p), None,
                                                     None, None, None, None)),
                 ("dpl_sparse_quant", L.dpl_sparse_quant(None, None, None, None, None, n, 1, n, 0, None, None)),
                 ("dpl_sparse_step", L.dpl_sparse_step(None, None, None, None, None, None, None, n, 1, n, 0, 1.0, 0.0, 0.0, 0.0,
                                                       1, 0, None, None)))
        for who, status in calls:
            assert status == -2, (who, n)
        assert L.dpl_round_init(None, None, n, 1, n, None, None, None) == -2
        assert L.dpl_last_error().decode() == "dpl_round_init: n must be in [1, 2^32 - 2^20]"
        assert L.dpl_sparse_step(None, None, None, None, None, None, None, n, 1, n, 0, 1.0, 0.0, 0.0, 0.0, 1, 0, None, None) == -2
        assert L.dpl_last_error().decode() == "dpl_sparse_step: n must be in [1, 2^32 - 2^20]"
    # the largest size passes the first check (nothing is launched: the second check refuses the made-up channel layout)
    assert L.dpl_round_quant(None, None, None, None, None, 2 ** 32 - 2 ** 20, 5, 2, 0, 1, None, None) == -2
    assert L.dpl_last_error().decode() == "dpl_round_quant: n must equal n_channels * inner"
    # the channel check still comes second, and a small call still runs
    assert L.dpl_round_quant(None, None, None, None, None, 12, 5, 2, 0, 1, None, None) == -2
    assert L.dpl_last_error().decode() == "dpl_round_quant: n must equal n_channels * inner"
    d = _edge(np.arange(12, dtype=F32), [1.0], [-127], [127], pc=False)
    wf, _ = k_init(d)
    assert_bits(host(wf), np.arange(12, dtype=F32), "small n")
