"""GPU parity: the HIP path (through the C ABI) against the reference-generated golden vectors and
against the CPU oracle on the same seeded inputs.

Bars: histogram counts, min/max, percentile clips: bit-exact.  OCTAV scale / clip thresholds: within
1e-5 (relative, with the same absolute floor) — the reference sums in fp32 pairwise order, the kernel
in fp64, so the last fp32 bit may differ.
"""
import json
import os
import warnings

import numpy as np
import pytest

import torch

from _cases import MINI_NET, make_tensor, mini_net_activations
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _close(a, b, tol=TOL):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        return np.all(both_nan | (a == b) | (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))   # (a == b: equal infinities)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    from dipoorlet_amd import _hip
    st, name, cus, mem = _hip.device_info()
    assert st == 0, name
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def kl(golden_dir):
    with open(os.path.join(golden_dir, "kernel_level.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, "kernel_level.npz"))


def test_minmax_golden(dev, kl):
    from dipoorlet_amd import ops
    meta, g = kl
    for c in meta["cases"]:
        x = torch.from_numpy(make_tensor(c["kind"], c["n"], c["seed"])).to(dev)
        got = ops.minmax(x).cpu().numpy()
        assert np.array_equal(got, g[c["key"] + "/minmax"], equal_nan=True), (c["key"], got, g[c["key"] + "/minmax"])


def test_minmax_nan_and_unaligned(dev):
    from dipoorlet_amd import ops
    x = make_tensor("normal", 70001, 3)
    base = torch.from_numpy(np.concatenate([np.zeros(3, np.float32), x])).to(dev)
    for off in (0, 1, 2, 3):  # 4-B aligned only: exercises the scalar head
        v = base[off:off + 70001 - 3]
        ref = O.minmax(base.cpu().numpy()[off:off + 70001 - 3])
        assert np.array_equal(ops.minmax(v.contiguous() if False else v).cpu().numpy(), np.array(ref))
    xn = x.copy()
    xn[12345] = np.nan
    got = ops.minmax(torch.from_numpy(xn).to(dev)).cpu().numpy()
    assert np.isnan(got).all()  # numpy max/min propagate NaN


def test_abs_hist_golden_bit_exact(dev, kl):
    from dipoorlet_amd import ops
    meta, g = kl
    for c in meta["cases"]:
        x = torch.from_numpy(make_tensor(c["kind"], c["n"], c["seed"])).to(dev)
        gmin0, gmax0 = g[c["key"] + "/minmax"]
        if c["kind"] == "with_nan":  # NaN range: np.histogram raises in the reference; flagged as status 1 here
            _, acc = ops.abs_hist(x, 2048, float(gmin0), float(gmax0))
            assert c["hist_raises"] and acc.range_status()["status"][0] == 1
            continue
        for bins in (2048, 1000):
            for scale in (1.0, 1.5):
                gmin, gmax = np.float32(gmin0 * np.float32(scale)), np.float32(gmax0 * np.float32(scale))
                tag = f"{c['key']}/hist_b{bins}_s{scale}"
                h, acc = ops.abs_hist(x, bins, float(gmin), float(gmax))
                hh = h.cpu().numpy()
                assert np.array_equal(hh, g[tag]), (tag, np.nonzero(hh != g[tag])[0][:10])
                for thr in (0.99999, 0.999):
                    clip = acc.hist_percentile(thr).cpu().numpy()[0]
                    assert np.array_equal(clip.view(np.uint32), g[f"{tag}_clip{thr}"].view(np.uint32)), (tag, thr)


def test_abs_hist_vs_numpy_random_ranges(dev):
    """Oracle-independent check straight against np.histogram, odd bin counts, NaN, values above range."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(11)
    for bins in (2048, 1000, 777, 64, 1, 16384):
        for trial in range(3):
            n = int(rng.integers(1, 300000))
            x = (rng.standard_normal(n) * rng.uniform(1e-3, 40)).astype(np.float32)
            if trial == 1:
                x[rng.integers(0, n, 5)] = np.nan
            dmax = np.float32(np.nanmax(np.abs(x)) * rng.choice([1.0, 1.25, 0.5]))
            ref, _ = np.histogram(np.abs(x), bins, (0, dmax))
            h, _ = ops.abs_hist(torch.from_numpy(x).to(dev), bins, 0.0, float(dmax))
            assert np.array_equal(h.cpu().numpy(), ref), (bins, trial, n)


def test_hist_prepare_flags_bad_ranges(dev):
    from dipoorlet_amd import ops
    x = torch.zeros(1024, device=dev)
    _, acc = ops.abs_hist(x, 2048, 0.0, float("inf"))
    assert acc.range_status()["status"][0] == 1
    _, acc = ops.abs_hist(x, 2048, 0.0, float("nan"))  # python max(nan, -min) keeps the NaN -> numpy raises
    assert acc.range_status()["status"][0] == 1
    _, acc = ops.abs_hist(x, 2048, float("nan"), 1.0)  # python max(1.0, nan) keeps 1.0 -> a valid range
    assert acc.range_status()["status"][0] == 0
    _, acc = ops.abs_hist(x, 2048, 0.0, 1e-42)  # denormal range: numpy raises "Too many bins"
    assert acc.range_status()["status"][0] == 2


def _same_steps(a, b):
    """Two forms walked the same iterate sequence: min / max identical, scales equal up to the ORDER in which atomically
    merged fp64 partial sums were added (the compaction and full-pass routes merge per-workgroup sums with atomics: one
    fp32 ulp at most, seen once in some hundred runs; a different iterate sequence differs by 1e-6 and more)."""
    return np.array_equal(a[..., 1:], b[..., 1:], equal_nan=True) and \
        np.allclose(a[..., 0], b[..., 0], rtol=2.4e-7, atol=0, equal_nan=True)


def _octav(ops, plan, tensors, dyn, form, states=None):
    """octav_batch; the exact-tail form is run three times on the same plan (cold, then with a threshold history): returned is
    the second call's result, checked against the other two."""
    got = ops.octav_batch(plan, tensors, dyn, states, form=form).cpu().numpy()
    if form == "tail":
        # the exact-tail form: the first call of a plan has no threshold history (lists from the bottom of the window and raises
        # the threshold on the fly), the later ones start from what the earlier calls asked for.  Where the list starts decides
        # which early iterates are bounds and which are exact, not where the walk ends: same fixed point, up to the stop rule
        # (|s' - s| < 1e-6) firing one step apart
        first = got
        got = ops.octav_batch(plan, tensors, dyn, states, form=form).cpu().numpy()
        again = ops.octav_batch(plan, tensors, dyn, states, form=form).cpu().numpy()
        for a in (first, again):
            assert np.array_equal(a[..., 1:], got[..., 1:], equal_nan=True)
            assert _close(a[..., 0], got[..., 0])
    return got


@pytest.mark.parametrize("form", ["tail", "bracket", "compact", "full"])
def test_octav_golden(dev, kl, form):
    """All forms against the reference's own outputs: exact tail / bounded bulk (the default), and the three that walk the
    reference's iterate sequence (two-read bracket, tail compaction, full re-reads)."""
    from dipoorlet_amd import ops
    meta, g = kl
    for c in meta["cases"]:
        x = torch.from_numpy(make_tensor(c["kind"], c["n"], c["seed"])).to(dev)
        plan = ops.TensorSetPlan([c["n"]], 1, dev)
        for deploy, dyn in (("trt", False), ("ti", True)):
            ref = g[f"{c['key']}/octav_{deploy}"]
            got = _octav(ops, plan, [x], dyn, form)[0, 0]
            assert _close(got[0], ref[0]), (c["key"], deploy, form, got, ref)
            assert np.array_equal(got[1:], ref[1:], equal_nan=True), (c["key"], got, ref)
            if form != "tail" and np.isfinite(ref[0]) and ref[0] != 0:
                # the forms that walk the reference's iterate sequence are PINNED to its values: one fp32 ulp (measured: 50 of 60
                # cases bit-equal, worst 9.6e-8; the atomically merged sums of 'compact' / 'full' may add an ulp) — a parity
                # regression cannot hide behind the 1e-5 the exact-tail form is allowed
                bound = 1.2e-7 if form == "bracket" else 2.4e-7
                assert abs(float(got[0]) - float(ref[0])) <= bound * abs(float(ref[0])), (c["key"], deploy, form, got, ref)


def test_octav_non_monotone_pairs_fall_back_to_full_passes(dev):
    """Degenerate tensors whose iterates oscillate (all non-zeros equal; two-level values) leave list mode;
    batched with ordinary tensors and odd, unaligned sizes."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(8)
    B = 3
    sizes = [4099, 70001, 1000, 33]
    tensors = []
    for t, n in enumerate(sizes):
        rows = []
        for b in range(B):
            if t == 0:
                x = np.where(rng.random(n) < 0.5, np.float32(2.0), np.float32(0.0)).astype(np.float32)
            elif t == 2:
                x = np.where(rng.random(n) < 0.9, np.float32(0.5), np.float32(-7.0)).astype(np.float32)
            else:
                x = make_tensor("relu" if b % 2 else "normal", n, 31 * t + b)
            rows.append(x)
        tensors.append(torch.from_numpy(np.stack(rows)).to(dev))
    plan = ops.TensorSetPlan(sizes, B, dev)
    a = ops.octav_batch(plan, tensors, False, form="compact").cpu().numpy()
    f = ops.octav_batch(plan, tensors, False, form="full").cpu().numpy()
    k = ops.octav_batch(plan, tensors, False, form="bracket").cpu().numpy()
    e = _octav(ops, plan, tensors, False, "tail")      # (refuses such pairs: the rescue / the compaction route finishes them)
    for t in range(len(sizes)):
        for b in range(B):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                s = O.octav_scale(tensors[t][b].cpu().numpy(), 1)
            assert _close(a[b, t, 0], s) and _close(f[b, t, 0], s) and _close(k[b, t, 0], s) \
                and _close(e[b, t, 0], s), (t, b, a[b, t], f[b, t], k[b, t], e[b, t], s)


def test_batched_tensor_set_vs_golden_pipeline_stats(dev, golden_dir):
    """The whole MINI_NET for all images in ONE batched launch per statistic."""
    from dipoorlet_amd import ops
    st = np.load(os.path.join(golden_dir, "pipeline_stats.npz"))
    N = 8
    names = [n for n, _, _ in MINI_NET]
    acts = [dict(mini_net_activations(i)) for i in range(N)]
    tensors = [torch.from_numpy(np.stack([acts[i][k] for i in range(N)])).to(dev) for k in names]
    plan = ops.TensorSetPlan([e for _, e, _ in MINI_NET], N, dev, chunk_elems=2048)
    acc = ops.CalibAccumulators(len(names), dev, 2048)
    acc.minmax_accumulate(plan, tensors)
    gmin, gmax = (t.cpu().numpy() for t in acc.finalize_minmax())
    acc.hist_prepare()
    acc.abs_hist_accumulate(plan, tensors)
    hist = acc.hist.cpu().numpy()
    oc = ops.octav_batch(plan, tensors, True).cpu().numpy()
    for t, k in enumerate(names):
        assert gmin[t] == st[f"{k}/min"].min() and gmax[t] == st[f"{k}/max"].max()
        assert np.array_equal(hist[t], st[f"{k}/hist"].sum(0)), k
        assert _close(oc[:, t, 0], st[f"{k}/octav_s_ti"]), (k, oc[:, t, 0], st[f"{k}/octav_s_ti"])
        assert np.array_equal(oc[:, t, 1], st[f"{k}/min"]) and np.array_equal(oc[:, t, 2], st[f"{k}/max"])


def test_accumulation_across_launches_equals_single_launch(dev):
    from dipoorlet_amd import ops
    n, B = 50000, 4
    xs = [torch.from_numpy(np.stack([make_tensor("relu", n, 10 * j + b) for b in range(B)])).to(dev)
          for j in range(3)]
    plan = ops.TensorSetPlan([n], B, dev)
    acc = ops.CalibAccumulators(1, dev, 2048)
    for x in xs:
        acc.minmax_accumulate(plan, [x])
    acc.finalize_minmax()
    acc.hist_prepare()
    for x in xs:
        acc.abs_hist_accumulate(plan, [x])
    allx = torch.cat(xs).cpu().numpy().ravel()
    lo, hi = O.minmax(allx)
    assert acc.gmin.item() == lo and acc.gmax.item() == hi
    assert np.array_equal(acc.hist[0].cpu().numpy(), O.abs_hist(allx, 2048, O.hist_dmax(lo, hi)))
    assert int(acc.hist.sum().item()) == allx.size  # checksum of counts: every element landed in a bin


def test_rowwise_minmax_and_fake_quant_golden(dev, golden_dir):
    from dipoorlet_amd import ops
    g = np.load(os.path.join(golden_dir, "qparam_level.npz"))
    for k, tr in (("conv.w", False), ("conv.b", False), ("gemm.w", False), ("deconv.w", True)):
        w = g[f"w/{k}"]
        if tr:
            w = w.transpose([1, 0, 2, 3])
        w2 = torch.from_numpy(np.ascontiguousarray(w.reshape(w.shape[0], -1))).to(dev)
        lo, hi = ops.rowwise_minmax(w2)
        assert np.array_equal(lo.cpu().numpy(), g[f"wmin/{k}"]) and np.array_equal(hi.cpu().numpy(), g[f"wmax/{k}"])
    x = torch.from_numpy(g["qa/x"]).to(dev)
    for i in range(4):
        scale, qlo, qhi = g[f"qa/{i}/p"]
        y = ops.fake_quant(x, torch.tensor([scale], dtype=torch.float32), torch.tensor([0], dtype=torch.int32),
                           int(qlo), int(qhi))
        # reference-owned torch fake quant (quant_acti): values equal; -0.0 vs +0.0 is not distinguished
        assert np.array_equal(y.cpu().numpy(), g[f"qa/{i}/y"]), i


def test_fake_quant_per_channel_and_zero_point_vs_oracle(dev):
    from dipoorlet_amd import ops
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 5, 7, 3)).astype(np.float32) * 3
    for axis in (0, 1):
        C_ = x.shape[axis]
        scale = rng.uniform(0.01, 0.1, C_).astype(np.float32)
        zp = rng.integers(0, 255, C_).astype(np.int32)
        y = ops.fake_quant(torch.from_numpy(x).to(dev), torch.from_numpy(scale), torch.from_numpy(zp), 0, 255,
                           axis=axis)
        ref = O.fake_quant_qdq(x, scale, zp, axis=axis, signed=False)
        assert np.array_equal(y.cpu().numpy(), ref), axis
    y = ops.fake_quant(torch.from_numpy(x).to(dev), torch.tensor([0.037]), torch.tensor([-5]), -128, 127)
    assert np.array_equal(y.cpu().numpy(), O.fake_quant_qdq(x, np.float32(0.037), -5, signed=True))


@pytest.mark.parametrize("shape,axis", [((64, 64, 3, 3), 0), ((512, 2048, 1, 1), 0), ((8, 256, 56, 56), 1)])
def test_fake_quant_per_channel_vectorised_kernel_vs_oracle(dev, shape, axis):
    """a12 (quantize.py:197-239, ada_quant_layer.py:28-36): the per-channel kernel every real Conv weight / activation takes
    — k_fake_quant_channel<true>: inner extent a multiple of 4 and 16-byte aligned buffers, one division per 16-byte vector —
    against the oracle, bit for bit; then the same data through an UNALIGNED view, which the dispatcher sends to
    k_fake_quant_channel<false>.  Zero points 0 / 3 / 191 / 255 (uint8) and their int8 storage forms, saturation at both
    ends, exact .5 ties (power-of-two scales: x / scale is exact), -0.0, values far outside the grid."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(sum(shape) + axis)
    C_ = shape[axis]
    inner = int(np.prod(shape[axis + 1:]))
    assert inner % 4 == 0                                   # -> the vectorised variant (fake_quant_kernels.hip dpl_fake_quant)
    scale = rng.uniform(0.01, 0.1, C_).astype(np.float32)
    scale[::3] = np.float32(2.0) ** rng.integers(-6, -2, scale[::3].size)          # power-of-two scales: exact ties
    x = rng.standard_normal(shape).astype(np.float32) * 4
    flat = x.reshape(-1)
    k = rng.integers(-300, 300, flat.size // 8).astype(np.float32)
    sc_full = np.broadcast_to(scale.reshape([-1 if i == axis else 1 for i in range(len(shape))]), shape).reshape(-1)
    idx = rng.choice(flat.size, k.size, replace=False)
    flat[idx] = (k + np.float32(0.5)) * sc_full[idx]                                # ties (exact where the scale is 2^-n)
    flat[rng.choice(flat.size, 64, replace=False)] = np.float32(1e6)                # saturates high
    flat[rng.choice(flat.size, 64, replace=False)] = np.float32(-1e6)               # saturates low
    flat[rng.choice(flat.size, 64, replace=False)] = np.float32(-0.0)
    xt = torch.from_numpy(x).to(dev)
    buf = torch.empty(x.size + 1, dtype=torch.float32, device=dev)
    x_un = buf[1:].view(shape)                              # 4-byte aligned only: forces k_fake_quant_channel<false>
    x_un.copy_(xt)
    assert xt.data_ptr() % 16 == 0 and x_un.data_ptr() % 16 != 0
    zps = np.array([0, 3, 191, 255], np.int32)
    for signed in (False, True):
        zp_u = zps[rng.integers(0, 4, C_)]
        zp = np.where(zp_u > 127, zp_u - 256, zp_u).astype(np.int32) if signed else zp_u
        qlo, qhi = (-128, 127) if signed else (0, 255)
        ref = O.fake_quant_qdq(x, scale, zp, axis=axis, signed=signed)
        assert (np.abs(ref).max() > 0) and np.isfinite(ref).all()
        for name, src in (("vectorised", xt), ("unaligned view", x_un)):
            y = ops.fake_quant(src, torch.from_numpy(scale), torch.from_numpy(zp), qlo, qhi, axis=axis)
            got = y.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, signed, shape,
                                                                               int((got.view(np.uint32) != ref.view(np.uint32)).sum()))


@pytest.mark.parametrize("shape,axis", [((4, 64, 56, 56), None), ((4, 64, 56, 56), 1), ((3, 32, 7, 7), 1), ((5, 1001), None), ((2, 6, 3), 1)])
def test_fake_quant_with_producer_relu_and_add_relu_vs_oracle(dev, shape, axis):
    """a12 + the merge-ReLU rule (quantize.py:50-55, 74-93): k_fake_quant<PRE> — the Q/DQ pair with its producer's ReLU, or residual
    Add + ReLU, applied on the way in — against the oracle's Q -> DQ of np.maximum(x, 0) / np.maximum(x + x2, 0), bit for bit: per
    tensor and per channel (rows of 3136 / 49 / 3 elements: whole vectors, vectors that straddle two channels, element by element),
    zero points != 0 on the uint8 grid and their int8 storage forms, saturation at both ends, exact .5 ties, -0.0, +-inf, sums that
    cancel to +-0 and sums that round; aligned buffers and 4-byte-aligned views."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(abs(hash((shape, axis))) % (1 << 31))
    n_ch = shape[axis] if axis is not None else 1
    scale = rng.uniform(0.01, 0.1, n_ch).astype(np.float32)
    scale[::3] = np.float32(2.0) ** rng.integers(-6, -2, scale[::3].size)
    x = (rng.standard_normal(shape) * 4).astype(np.float32)
    x2 = (rng.standard_normal(shape) * 4).astype(np.float32)
    f, f2 = x.reshape(-1), x2.reshape(-1)
    sc_full = (np.broadcast_to(scale.reshape([-1 if i == axis else 1 for i in range(len(shape))]), shape).reshape(-1) if axis is not None
               else np.full(f.size, scale[0], np.float32))
    m = max(4, f.size // 8)
    idx = rng.choice(f.size, m, replace=False)
    f[idx] = (rng.integers(0, 300, m).astype(np.float32) + np.float32(0.5)) * sc_full[idx]        # ties
    sp = rng.choice(f.size, min(f.size, 40), replace=False)
    f[sp[0:8]] = np.float32(1e6)
    f[sp[8:16]] = np.float32(-1e6)
    f[sp[16:24]] = np.float32(-0.0)
    f[sp[24:28]] = np.float32(np.inf)
    f[sp[28:32]] = np.float32(-np.inf)
    f2[sp[28:32]] = np.float32(1.0)                       # (-inf + 1: no NaN from inf - inf)
    f2[sp[24:28]] = np.float32(1.0)
    f2[sp[32:36]] = -f[sp[32:36]]                         # x + x2 = +0 exactly
    f2[sp[36:40]] = np.float32(1e-9)                      # absorbed by the rounding of the sum
    xt, x2t = torch.from_numpy(x).to(dev), torch.from_numpy(x2).to(dev)
    buf = torch.empty(2 * (x.size + 1), dtype=torch.float32, device=dev)
    xu, x2u = buf[1:x.size + 1].view(shape), buf[x.size + 2:2 * x.size + 2].view(shape)
    xu.copy_(xt)
    x2u.copy_(x2t)
    zps = np.array([0, 3, 128, 191, 255], np.int32)
    with np.errstate(invalid="ignore"):
        relu, add_relu = np.maximum(x, np.float32(0)), np.maximum((x + x2).astype(np.float32), np.float32(0))
    for signed in (False, True):
        zp_u = zps[rng.integers(0, 5, n_ch)]
        zp = np.where(zp_u > 127, zp_u - 256, zp_u).astype(np.int32) if signed else zp_u
        qlo, qhi = (-128, 127) if signed else (0, 255)
        sc_t, zp_t = torch.from_numpy(scale).to(dev), torch.from_numpy(zp).to(dev)
        want = {None: O.fake_quant_qdq(x, scale, zp, axis=axis, signed=signed),
                "relu": O.fake_quant_qdq(relu, scale, zp, axis=axis, signed=signed),
                "add_relu": O.fake_quant_qdq(add_relu, scale, zp, axis=axis, signed=signed)}
        for tag, a, b in (("aligned", xt, x2t), ("unaligned", xu, x2u)):
            for pre in (None, "relu", "add_relu"):
                y = ops.fake_quant(a, sc_t, zp_t, qlo, qhi, axis=axis, pre=pre, x2=b if pre == "add_relu" else None)
                got = y.cpu().numpy()
                bad = int((got.view(np.uint32) != want[pre].view(np.uint32)).sum())
                assert bad == 0, (tag, pre, signed, shape, axis, bad)
                # ... and what the two (three) launches of the unfused chain write
                if pre is not None:
                    chain = ops.fake_quant(torch.relu(a if pre == "relu" else a + b).contiguous(), sc_t, zp_t, qlo, qhi, axis=axis)
                    assert torch.equal(chain, y), (tag, pre)
    with pytest.raises(Exception):
        ops.fake_quant(xt, sc_t, zp_t, qlo, qhi, axis=axis, pre="add_relu", x2=x2t.reshape(-1)[:-1])
    with pytest.raises(Exception):
        ops.fake_quant(xt, sc_t, zp_t, qlo, qhi, axis=axis, pre="add_relu")


# ---- the argument boundary of ops.fake_quant / fake_quant_fp8 / channel_diff_sum: negative axes, out=, acc=
# [7, 300]: 300 channels on the last axis (inner = 1), the element path's step of 256 wraps; [2, 3, 1025]: 6150 elements, two
# workgroup chunks of 3072, the second starting inside a row at channel 3072 % 1025; [4, 6, 3]: inner = 3; [5, 8, 7, 7]: axis -4 is
# axis 0, inner = 392, whole vectors within a row
NEGATIVE_AXES = [((7, 300), -1), ((2, 3, 1025), -1), ((4, 6, 3), -2), ((5, 8, 7, 7), -4)]


def _fq_edge_inputs(shape, axis, seed):
    """(x, x2, scale) with the values the neighbouring tests plant: exact ties of the integer grid and of E4M3 under power-of-two
    scales ((k + 0.5) * scale; odd integers in [16, 32) * scale), +-1e6, -0.0, +-inf (x2 = 1 there: no inf - inf), sums that cancel."""
    rng = np.random.default_rng(seed)
    n_ch = shape[axis]
    scale = rng.uniform(0.01, 0.1, n_ch).astype(np.float32)
    scale[::3] = np.float32(2.0) ** rng.integers(-6, -2, scale[::3].size)
    x = (rng.standard_normal(shape) * 4).astype(np.float32)
    x2 = (rng.standard_normal(shape) * 4).astype(np.float32)
    f, f2 = x.reshape(-1), x2.reshape(-1)
    sc_full = np.broadcast_to(scale.reshape([-1 if i == axis % len(shape) else 1 for i in range(len(shape))]), shape).reshape(-1)
    m = max(8, f.size // 8)
    idx = rng.choice(f.size, m, replace=False)
    f[idx[:m // 2]] = (rng.integers(0, 300, m // 2).astype(np.float32) + np.float32(0.5)) * sc_full[idx[:m // 2]]
    f[idx[m // 2:]] = (2 * rng.integers(8, 16, m - m // 2) + 1).astype(np.float32) * sc_full[idx[m // 2:]]
    sp = rng.choice(f.size, 40, replace=False)
    f[sp[0:8]] = np.float32(1e6)
    f[sp[8:16]] = np.float32(-1e6)
    f[sp[16:24]] = np.float32(-0.0)
    f[sp[24:28]] = np.float32(np.inf)
    f[sp[28:32]] = np.float32(-np.inf)
    f2[sp[24:32]] = np.float32(1.0)
    f2[sp[32:36]] = -f[sp[32:36]]
    f2[sp[36:40]] = np.float32(1e-9)
    return x, x2, scale


def _fq_pre_inputs(x, x2):
    """What the producer's ReLU hands the pair: negative values become +0 and a -0 stays -0, as torch.relu and fq_pre have it
    (np.maximum(-0.0, 0) may return either zero, and E4M3 keeps a zero's sign: tests/test_fp8_gpu.py)."""
    def relu(v):
        return np.where(v < 0, np.float32(0), v).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return {None: x, "relu": relu(x), "add_relu": relu((x + x2).astype(np.float32))}


def _off_by_4_bytes(t):
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4
    return v


def _bits_differ(got, want):
    got, want = np.ascontiguousarray(got.cpu().numpy()), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("fmt", ["int", "e4m3"])
@pytest.mark.parametrize("shape,axis", NEGATIVE_AXES)
def test_fake_quant_negative_axis_vs_oracle(dev, shape, axis, fmt):
    """A channel axis counted from the end (ONNX QuantizeLinear allows it) is the axis it names: ops.fake_quant / fake_quant_fp8
    with axis = -k and with axis = dim - k give the same bits, the oracle's (np_oracle.fake_quant_qdq, tests/fp8_model.py) — on the
    integer grid with non-zero zero points (uint8 and their int8 storage forms) and on E4M3, with the producer's ReLU / Add + ReLU,
    on a 16-byte-aligned buffer and on a view 4 bytes off.  The first two shapes also through the torch ops."""
    import dipoorlet_amd.torch_ops  # noqa: F401
    import fp8_model
    from dipoorlet_amd import ops
    front = axis % len(shape)
    x, x2, scale = _fq_edge_inputs(shape, axis, 1000 * len(shape) + shape[-1])
    src = _fq_pre_inputs(x, x2)
    xt, x2t, sc_t = torch.from_numpy(x).to(dev), torch.from_numpy(x2).to(dev), torch.from_numpy(scale).to(dev)
    placed = (("aligned", xt, x2t), ("4 bytes off", _off_by_4_bytes(xt), _off_by_4_bytes(x2t)))
    through_torch_ops = shape in ((7, 300), (2, 3, 1025))
    rng = np.random.default_rng(7)
    for signed in ((False, True) if fmt == "int" else (None,)):
        if fmt == "int":
            zp_u = np.array([3, 128, 191, 255], np.int32)[rng.integers(0, 4, scale.size)]
            zp = np.where(zp_u > 127, zp_u - 256, zp_u).astype(np.int32) if signed else zp_u
            zp_t = torch.from_numpy(zp).to(dev)
            qlo, qhi = (-128, 127) if signed else (0, 255)
            want = {pre: O.fake_quant_qdq(v, scale, zp, axis=axis, signed=signed) for pre, v in src.items()}
            assert all(np.array_equal(w, O.fake_quant_qdq(src[pre], scale, zp, axis=front, signed=signed)) for pre, w in want.items())

            def run(a, b, ax, pre):
                return ops.fake_quant(a, sc_t, zp_t, qlo, qhi, axis=ax, pre=pre, x2=b if pre == "add_relu" else None)
            torch_op = {None: lambda a, b, ax: torch.ops.dipoorlet.fake_quant(a, sc_t, zp_t, ax, qlo, qhi),
                        "relu": lambda a, b, ax: torch.ops.dipoorlet.fake_quant_relu(a, sc_t, zp_t, ax, qlo, qhi),
                        "add_relu": lambda a, b, ax: torch.ops.dipoorlet.fake_quant_add_relu(a, b, sc_t, zp_t, ax, qlo, qhi)}
        else:
            want = {pre: fp8_model.fake_quant_fp8(v, scale, axis=axis) for pre, v in src.items()}

            def run(a, b, ax, pre):
                return ops.fake_quant_fp8(a, sc_t, axis=ax, pre=pre, x2=b if pre == "add_relu" else None)
            torch_op = {None: lambda a, b, ax: torch.ops.dipoorlet.fake_quant_fp8(a, sc_t, ax)}
        for tag, a, b in placed:
            for pre in (None, "relu", "add_relu"):
                y_neg, y_front = run(a, b, axis, pre), run(a, b, front, pre)
                where = (tag, pre, signed, shape, axis)
                assert torch.equal(y_neg.view(torch.int32), y_front.view(torch.int32)), where
                assert _bits_differ(y_neg, want[pre]) == 0, (where, _bits_differ(y_neg, want[pre]))
                assert _bits_differ(y_front, want[pre]) == 0, (where, _bits_differ(y_front, want[pre]))
                if through_torch_ops and pre in torch_op:
                    for ax in (axis, front):
                        assert _bits_differ(torch_op[pre](a, b, ax), want[pre]) == 0, (where, ax, "torch op")


@pytest.mark.parametrize("fmt", ["int", "fp8"])
def test_fake_quant_set_offset_member_and_wide_last_axis_channels(dev, fmt):
    """FakeQuantSet (dpl_fake_quant_items / dpl_fake_quant_fp8_items) with one member that is a view 4 bytes off a 16-byte boundary
    (element by element) and one per-channel member with inner = 1 and 300 channels — more than the 256 the element path advances
    per step, 6 x 300 elements: the step wraps, rows start at every phase — beside an aligned per-channel one with whole vectors:
    the oracle's bits, out of place and in place."""
    import fp8_model
    from dipoorlet_amd import ops
    B = 2
    shapes = [(B, 5, 7, 7), (B, 3, 300, 1), (B, 8, 4, 4)]      # member t seen as [B * shape[1], C = shape[2], inner = shape[3]]
    rng = np.random.default_rng(77)
    plan = ops.TensorSetPlan([int(np.prod(s[1:])) for s in shapes], B, dev)
    xs, params, want = [], [], []
    for t, s in enumerate(shapes):
        view = (s[0] * s[1], s[2], s[3])
        x, _, scale = _fq_edge_inputs(view, 1, 300 + t)
        xt = torch.from_numpy(x).to(dev)
        xs.append(_off_by_4_bytes(xt) if t == 0 else xt)
        if fmt == "fp8":
            params.append((torch.from_numpy(scale), s[3]))
            want.append(fp8_model.fake_quant_fp8(x, scale, axis=1))
        else:
            signed = t == 2
            zp_u = np.array([3, 128, 191, 255], np.int32)[rng.integers(0, 4, scale.size)]
            zp = np.where(zp_u > 127, zp_u - 256, zp_u).astype(np.int32) if signed else zp_u
            params.append((torch.from_numpy(scale), torch.from_numpy(zp), s[3], *((-128, 127) if signed else (0, 255))))
            want.append(O.fake_quant_qdq(x, scale, zp, axis=1, signed=signed))
    assert xs[0].data_ptr() % 16 == 4 and shapes[1][2] > 256 and shapes[1][3] == 1
    fset = ops.FakeQuantSet(plan, params, fmt=fmt)
    ys = fset(xs)
    for t in range(len(shapes)):
        assert _bits_differ(ys[t], want[t]) == 0, (fmt, t, "out of place", _bits_differ(ys[t], want[t]))
    again = [_off_by_4_bytes(x.clone()) if t == 0 else x.clone() for t, x in enumerate(xs)]
    assert fset(again, out=again) is again
    for t in range(len(shapes)):
        assert _bits_differ(again[t], want[t]) == 0, (fmt, t, "in place", _bits_differ(again[t], want[t]))


GUARD_VALUE = -777.0


def _guarded(dev, numel, dtype, device=None):
    """A block of 3 * numel elements of GUARD_VALUE: whatever a refused target is cut from it, an unchecked launch that writes `numel`
    elements (of this or a narrower type) from the target's first element on stays inside the block.  A host block is pinned:
    page-locked host memory is mapped into the device's address space, so even there such a launch writes memory the test owns."""
    if device == "cpu":
        return torch.full((3 * numel,), GUARD_VALUE, dtype=dtype).pin_memory()
    return torch.full((3 * numel,), GUARD_VALUE, dtype=dtype, device=dev)


@pytest.mark.parametrize("entry", ["fake_quant", "fake_quant_fp8"])
def test_fake_quant_refuses_an_out_it_cannot_fill_and_an_axis_out_of_range(dev, entry):
    """out= of ops.fake_quant / fake_quant_fp8 must be a contiguous fp32 tensor of x's shape on x's device (x itself is allowed):
    one element short, fp16, transposed or on the host it is refused with a DipoorletHipError and nothing is written — every
    refused target is a view into a block of guard values three times the size of what the kernel writes, so that an unchecked
    launch gives a wrong answer inside memory this test owns.  An axis of dim or -dim - 1 is refused too."""
    from dipoorlet_amd import _hip, ops
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((6, 8)).astype(np.float32)).to(dev)
    n = x.numel()
    sc1 = torch.tensor([0.05], device=dev)
    scc = torch.from_numpy(rng.uniform(0.01, 0.1, 8).astype(np.float32)).to(dev)
    zp1, zpc = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

    def call(scale, zp, **kw):
        if entry == "fake_quant":
            return ops.fake_quant(x, scale, zp, -128, 127, **kw)
        return ops.fake_quant_fp8(x, scale, **kw)
    blocks = {"one element short": _guarded(dev, n, torch.float32), "fp16": _guarded(dev, 2 * n, torch.float16),
              "transposed": _guarded(dev, n, torch.float32), "on the host": _guarded(dev, n, torch.float32, device="cpu")}
    targets = {"one element short": blocks["one element short"][n:2 * n - 1],
               "fp16": blocks["fp16"][2 * n:3 * n].view(6, 8),
               "transposed": blocks["transposed"][n:2 * n].view(8, 6).t(),
               "on the host": blocks["on the host"][n:2 * n].view(6, 8)}
    for why, out in targets.items():
        with pytest.raises(_hip.DipoorletHipError):
            call(sc1, zp1, out=out)
        torch.cuda.synchronize()
        assert bool((blocks[why] == GUARD_VALUE).all()), (entry, why, "the refused out was written")
    for axis in (2, -3):
        good = _guarded(dev, n, torch.float32)
        with pytest.raises(_hip.DipoorletHipError):
            call(scc, zpc, axis=axis, out=good[n:2 * n].view(6, 8))
        torch.cuda.synchronize()
        assert bool((good == GUARD_VALUE).all()), (entry, axis)
    # what stays allowed: a contiguous fp32 view of x's shape, and x itself
    ok = _guarded(dev, n, torch.float32)
    want = call(scc, zpc, axis=1).clone()
    assert call(scc, zpc, axis=-1, out=ok[n:2 * n].view(6, 8)).data_ptr() == ok[n:].data_ptr()
    assert torch.equal(ok[n:2 * n].view(6, 8), want) and bool((ok[:n] == GUARD_VALUE).all()) and bool((ok[2 * n:] == GUARD_VALUE).all())
    assert call(scc, zpc, axis=1, out=x) is x and torch.equal(x, want)


def test_channel_diff_sum_refuses_an_acc_it_cannot_fill(dev):
    """acc= of ops.channel_diff_sum must be a contiguous fp64 tensor of C elements on a's device: the kernel adds C fp64 values at
    it.  fp32 or C - 1 elements: refused, and the guard block the target is cut from stays as it was."""
    from dipoorlet_amd import _hip, ops
    rng = np.random.default_rng(4)
    a = torch.from_numpy(rng.standard_normal((3, 6, 5)).astype(np.float32)).to(dev)
    b = torch.zeros_like(a)
    C_ = 6
    blocks = {"fp32": _guarded(dev, 2 * C_, torch.float32), "C - 1 elements": _guarded(dev, C_, torch.float64)}
    targets = {"fp32": blocks["fp32"][2 * C_:3 * C_], "C - 1 elements": blocks["C - 1 elements"][C_:2 * C_ - 1]}
    for why, acc in targets.items():
        with pytest.raises(_hip.DipoorletHipError):
            ops.channel_diff_sum(a, b, acc)
        torch.cuda.synchronize()
        assert bool((blocks[why] == GUARD_VALUE).all()), (why, "the refused acc was written")
    ok = _guarded(dev, C_, torch.float64)
    acc = ok[C_:2 * C_]
    acc.zero_()
    assert ops.channel_diff_sum(a, b, acc) is acc
    np.testing.assert_allclose(acc.cpu().numpy(), a.double().sum((0, 2)).cpu().numpy(), rtol=1e-12, atol=1e-12)
    assert bool((ok[:C_] == GUARD_VALUE).all()) and bool((ok[2 * C_:] == GUARD_VALUE).all())


def test_cos_accumulate(dev):
    from dipoorlet_amd import ops
    a = make_tensor("normal", 123457, 1)
    b = (a + make_tensor("normal", 123457, 2) * np.float32(0.05)).astype(np.float32)
    acc = torch.zeros(3, dtype=torch.float64, device=dev)
    ops.cos_accumulate(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), acc)
    ab, aa, bb = acc.cpu().numpy()
    cos = ab / np.sqrt(aa) / np.sqrt(bb)
    assert abs(cos - float(O.cos_similarity(a, b))) < 1e-5


def test_full_size_properties_resnet50_shapes(dev):
    """BASELINE-size inputs: size-independent properties instead of an element-wise oracle."""
    from dipoorlet_amd import ops
    from dipoorlet_amd.synthetic import resnet50_tensor_elems, synth_activations
    elems = resnet50_tensor_elems()
    B = 4
    tensors = synth_activations(elems, B, dev, seed=99)
    plan = ops.TensorSetPlan(elems, B, dev)
    acc = ops.CalibAccumulators(len(elems), dev, 2048)
    acc.minmax_accumulate(plan, tensors)
    gmin, gmax = acc.finalize_minmax()
    acc.hist_prepare()
    acc.abs_hist_accumulate(plan, tensors)
    # (1) checksum of checksums: every element is counted exactly once
    per_tensor = acc.hist.sum(1).cpu().numpy()
    assert np.array_equal(per_tensor, np.array(elems, np.int64) * B)
    # (2) ranges agree with torch's own reductions
    tmin = torch.stack([t.min() for t in tensors])
    tmax = torch.stack([t.max() for t in tensors])
    assert torch.equal(gmin, tmin) and torch.equal(gmax, tmax)
    # (3) idempotence / linearity: a second accumulation of the same batch doubles every count
    h1 = acc.hist.clone()
    acc.abs_hist_accumulate(plan, tensors)
    assert torch.equal(acc.hist, 2 * h1)
    # (4) the last occupied bin holds the range maximum; nothing beyond the range was dropped
    # (5) spot-check three tensors element-wise against the oracle
    for t in (0, 5, len(elems) - 1):
        x = tensors[t].cpu().numpy().ravel()
        lo, hi = O.minmax(x)
        assert np.array_equal(h1[t].cpu().numpy(), O.abs_hist(x, 2048, O.hist_dmax(lo, hi)))
    # (6) OCTAV on the batch: spot-check pairs against the oracle
    oc = ops.octav_batch(plan, tensors, False).cpu().numpy()
    for (b, t) in ((0, 0), (1, 7), (3, len(elems) - 1), (2, 40)):
        x = tensors[t][b].cpu().numpy().ravel()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            s = O.octav_scale(x, 1)
        assert _close(oc[b, t, 0], s), (b, t, oc[b, t], s)


def test_abs_hist_edge_stress_all_bin_counts_and_magnitudes(dev):
    """The one-sided bin search (biased reciprocal + single decrement test) must equal np.histogram for
    values ON the fp32 bin edges and one ulp to either side, for any bin count up to the LDS limit and
    ranges from 1e-30 to 1e30 (tiny ranges take the exact-divide path, checked too)."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(2024)
    cases = [(2048, 6.1), (16384, 3.3e-3), (16384, 9.7e29), (1000, 1e-29), (777, 4.2e12), (3, 1.0), (1, 5.0),
             (2047, 1.1754944e-38 * 4096), (4096, 1e-33), (1024, 2.5e-36)]
    for _ in range(12):
        cases.append((int(rng.integers(2, 16385)), float(10.0 ** rng.uniform(-25, 25))))
    for bins, dm in cases:
        dmax = np.float32(dm)
        step = np.float32(dmax / np.float32(bins))
        i = rng.integers(0, bins + 1, 60000).astype(np.float32)
        e = (i * step).astype(np.float32)
        e[i == bins] = dmax
        lo = np.nextafter(e, np.float32(-np.inf))
        hi = np.nextafter(e, np.float32(np.inf))
        x = np.concatenate([e, lo, hi, rng.uniform(0, float(dmax), 60000).astype(np.float32),
                            np.array([0.0, -0.0, float(dmax), -float(dmax)], np.float32)])
        x = np.clip(x, 0, None).astype(np.float32) * rng.choice(np.array([-1, 1], np.float32), x.size)
        try:
            ref, _ = np.histogram(np.abs(x), bins, (0, dmax))
        except ValueError:
            _, acc = ops.abs_hist(torch.from_numpy(x).to(dev), bins, 0.0, float(dmax))
            assert acc.range_status()["status"][0] != 0, (bins, dm)
            continue
        h, acc = ops.abs_hist(torch.from_numpy(x).to(dev), bins, 0.0, float(dmax))
        assert acc.range_status()["status"][0] == 0, (bins, dm)
        got = h.cpu().numpy()
        assert np.array_equal(got, ref), (bins, dm, int(acc.range_status()["exact_div"][0]),
                                          np.nonzero(got != ref)[0][:8], int(np.abs(got - ref).sum()))


def test_empty_and_tiny_spans(dev):
    from dipoorlet_amd import ops
    plan = ops.TensorSetPlan([1, 3, 5], 2, dev)
    xs = [torch.tensor([[1.5], [-2.5]], device=dev), torch.tensor([[0., 1., 2.], [3., -4., 0.]], device=dev),
          torch.zeros(2, 5, device=dev)]
    acc = ops.CalibAccumulators(3, dev, 64)
    acc.minmax_accumulate(plan, xs)
    lo, hi = acc.finalize_minmax()
    assert lo.tolist() == [-2.5, -4.0, 0.0] and hi.tolist() == [1.5, 3.0, 0.0]
    acc.hist_prepare()
    acc.abs_hist_accumulate(plan, xs)
    for t, x in enumerate(xs):
        ref, _ = np.histogram(np.abs(x.cpu().numpy()), 64, (0, np.float32(max(hi[t].item(), -lo[t].item()))))
        assert np.array_equal(acc.hist[t].cpu().numpy(), ref)
    oc = ops.octav_batch(plan, xs, False).cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for t, x in enumerate(xs):
            for b in range(2):
                s = O.octav_scale(x[b].cpu().numpy(), 1)
                assert _close(oc[b, t, 0], s), (t, b, oc[b, t], s)


@pytest.mark.parametrize("form", ["tail", "bracket"])
def test_octav_bracket_routes(dev, form):
    """The histogram forms on data that exercises each route: ordinary tensors (bracket), a flat distribution whose
    bracket explodes, values beyond the 2^14 window, a huge dynamic range, all in one batched launch."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(17)
    B, n = 2, 300000
    mk = [lambda: rng.standard_normal(n).astype(np.float32) * 3,
          lambda: rng.uniform(-3, 5, n).astype(np.float32),                       # flat: goes to the compaction route
          lambda: (rng.standard_normal(n) * 9000).astype(np.float32),             # values >= 2^14
          lambda: np.maximum(rng.standard_normal(n), 0).astype(np.float32) * 1e-3,
          lambda: (rng.laplace(0, 1, n) * np.exp(rng.uniform(-6, 6, n))).astype(np.float32),
          lambda: np.where(rng.random(n) < 0.999, 0, rng.standard_normal(n)).astype(np.float32)]
    tensors = [torch.from_numpy(np.stack([f() for _ in range(B)])).to(dev) for f in mk]
    plan = ops.TensorSetPlan([n] * len(mk), B, dev)
    got = _octav(ops, plan, tensors, False, form)
    for t in range(len(mk)):
        for b in range(B):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                s = O.octav_scale(tensors[t][b].cpu().numpy(), 1)
            assert _close(got[b, t, 0], s), (t, b, got[b, t], s)


@pytest.mark.parametrize("form", ["tail", "bracket"])
def test_octav_exact_walk_restart_path(dev, form):
    _restart_path(dev, form)


def _restart_path(dev, form):
    """An iterate that leaves the bracket's bins makes the exact walk hand the pair to the compaction route.  That is
    rare by construction, so the C-ABI test hook rejects every second pair on purpose: the results must not change."""
    from dipoorlet_amd import _hip, ops
    rng = np.random.default_rng(23)
    B, sizes = 3, [150528, 40000, 802816, 1000]
    tensors = [torch.from_numpy(np.stack([(rng.standard_normal(n) * (1 + t)).astype(np.float32) if t % 2 == 0 else
                                          np.maximum(rng.standard_normal(n), 0).astype(np.float32) * 2.5
                                          for _ in range(B)])).to(dev) for t, n in enumerate(sizes)]
    plan = ops.TensorSetPlan(sizes, B, dev)
    want = _octav(ops, plan, tensors, False, form)     # (exact tail: also warms the threshold history up, so that only the hook fails pairs)
    states = torch.empty((plan.n_pairs + 1) * 80, dtype=torch.uint8, device=dev)

    def hooked(rescue_fail):
        old = _hip.lib().dpl_test_hook_exact_fail_every(2)
        old_r = _hip.lib().dpl_test_hook_rescue_fail_every(rescue_fail)
        try:
            got = ops.octav_batch(plan, tensors, False, states, form=form).cpu().numpy()
            ctl = _hip.OctavState.from_buffer_copy(states.cpu().numpy()[-80:].tobytes())
        finally:
            _hip.lib().dpl_test_hook_exact_fail_every(old)
            _hip.lib().dpl_test_hook_rescue_fail_every(old_r)
        return got, ctl

    got, ctl = hooked(0)
    if form == "tail":
        # the exact-tail form RESCUES a rejected pair (its exact bracket, a re-read of that pair alone, a second walk); only
        # the pairs that gather their whole window anyway (here: the 1000-element tensor) go straight to the compaction route
        assert int(ctl.len0) + int(ctl.cnt_le) >= plan.n_pairs // 2 and int(ctl.len0) >= plan.n_pairs // 4
        assert int(ctl.len1) >= int(ctl.len0)                # units of the re-read
        got2, ctl2 = hooked(2)                               # ... and when the rescue walk rejects them too: compaction route
        assert int(ctl2.cnt_le) >= plan.n_pairs // 2
        assert _close(got2[..., 0], want[..., 0])
    else:
        assert int(ctl.cnt_le) == plan.n_pairs // 2          # control block: pairs that took the compaction route
    # (exact tail: a rescued pair walks the reference's whole iterate sequence, an accepted one only its end: same fixed point)
    assert _same_steps(got, want) if form != "tail" else (_close(got[..., 0], want[..., 0]) and np.array_equal(got[..., 1:], want[..., 1:]))
    for t in range(len(sizes)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert _close(got[0, t, 0], O.octav_scale(tensors[t][0].cpu().numpy(), 1))


def test_gemm_small(dev):
    """dpl_gemm_small (the classifier head of a convolutional network: csrc/gemm_small.hip) against numpy in fp64: ResNet-50's
    head at the default batch (a transposed VIEW of the [N, K] weight, as an ONNX Gemm with transB = 1 gives), sizes that are not
    multiples of the tile, every bias broadcast, alpha / beta, K = 0, K cut into 1 ... 64 splits (some of them empty); the result does not depend on the launch (bit-equal
    repeats) nor a row on the batch it came in; a product above DPL_GEMM_SMALL_MAX is refused."""
    from dipoorlet_amd import _hip, ops
    rng = np.random.default_rng(61)
    for M, K, N, trans_b, bias_kind, alpha, beta in [(64, 2048, 1000, True, "n", 1.0, 1.0), (1, 1, 1, False, None, 1.0, 1.0),
                                                     (33, 65, 31, False, "1n", 0.5, 2.0), (7, 300, 129, True, "mn", 1.0, -1.0),
                                                     (32, 32, 64, False, "m1", 1.0, 1.0), (5, 0, 9, False, "n", 1.0, 1.0),
                                                     (200, 1280, 1001, True, "n", 1.0, 1.0), (64, 512, 10, True, None, 1.0, 1.0),
                                                     (8, 8200, 64, False, "n", 1.0, 1.0), (300, 96, 600, False, "1n", 1.0, 1.0)]:
        a = rng.standard_normal((M, K)).astype(np.float32)
        w = rng.standard_normal((N, K) if trans_b else (K, N)).astype(np.float32)
        bias = {None: None, "n": (N,), "1n": (1, N), "mn": (M, N), "m1": (M, 1)}[bias_kind]
        bias = None if bias is None else rng.standard_normal(bias).astype(np.float32)
        wt = torch.from_numpy(w).to(dev)
        b = wt.t() if trans_b else wt
        bt = None if bias is None else torch.from_numpy(bias).to(dev)
        got = ops.gemm_small(torch.from_numpy(a).to(dev), b, bt, alpha, beta)
        again = ops.gemm_small(torch.from_numpy(a).to(dev), b, bt, alpha, beta)
        want = alpha * (a.astype(np.float64) @ (w.T if trans_b else w).astype(np.float64))
        if bias is not None:
            want = want + beta * bias.astype(np.float64)
        assert got.shape == (M, N) and torch.equal(got, again)
        scale = np.sqrt(max(K, 1)) * abs(alpha) + abs(beta)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=2e-6 * scale * max(1.0, np.sqrt(K) / 8))
    # a row of the result is the same sum whatever batch it came in (the number of splits of K depends on N and K only)
    a = torch.randn(120, 2048, device=dev)
    w = torch.randn(1000, 2048, device=dev)
    c = torch.randn(1000, device=dev)
    full = ops.gemm_small(a, w.t(), c)
    for lo, hi in ((0, 1), (3, 7), (0, 64), (64, 120), (17, 50)):
        assert torch.equal(ops.gemm_small(a[lo:hi], w.t(), c), full[lo:hi]), (lo, hi)
    big = torch.zeros(1 << 10, 1 << 10, device=dev)
    with pytest.raises(_hip.DipoorletHipError):
        ops.gemm_small(big, torch.zeros(1 << 10, 1 << 9, device=dev))        # 2^29 multiply-adds
    with pytest.raises(_hip.DipoorletHipError):
        ops.gemm_small(torch.zeros(4, 8), torch.zeros(8, 2, device=dev))     # a CPU tensor


def test_executor_small_products_need_no_blas(dev, monkeypatch):
    """The executor's Gemm / MatMul take ops.gemm_small for a small product (same values as the library's to fp32 rounding) and
    hipBLASLt for a large one or with DPL_GEMM_SMALL=0; GraphSession.needs_blas says which at session build."""
    from dipoorlet_amd import executor, models
    from dipoorlet_amd.executor import GraphSession
    g = models.resnet18(num_classes=37)
    x = torch.randn(8, 3, 224, 224, device=dev)
    s = GraphSession(g, device=dev)
    assert not s.needs_blas(64) and s.needs_blas(1 << 20)
    feeds = {s.input_names[0]: x}
    b = s.run(feeds)[-1]                           # (the graph's last tensor: the Gemm's output)
    monkeypatch.setenv("DPL_GEMM_SMALL", "0")
    assert s.needs_blas(1)
    a = s.run(feeds)[-1]
    monkeypatch.delenv("DPL_GEMM_SMALL")
    assert a.shape == b.shape == (8, 37) and float(a.abs().max()) > 0
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5 * float(a.abs().max()))
    # MatMul with leading axes: [2, 5, 16] x [16, 12]
    w = torch.randn(16, 12, device=dev)
    y = torch.randn(2, 5, 16, device=dev)
    torch.testing.assert_close(executor._OPS["MatMul"](None, None, y, w), torch.matmul(y, w), rtol=1e-5, atol=1e-5)


def test_channel_diff_sum(dev):
    """dpl_channel_diff_sum (bias correction's mean(fp - q) per channel) against numpy in fp64: conv maps with rows of
    every alignment class, a Gemm output, accumulation over several chunks."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(29)
    for shape in ((5, 7, 14, 14), (3, 6, 7, 7), (2, 9, 5, 13), (4, 300), (2, 3, 64, 64), (1, 1, 3)):
        a = rng.standard_normal(shape).astype(np.float32)
        b = (a + rng.standard_normal(shape).astype(np.float32) * 1e-2).astype(np.float32)
        axes = tuple(i for i in range(len(shape)) if i != 1)
        want = (a.astype(np.float64) - b.astype(np.float64)).sum(axis=axes)
        acc = ops.channel_diff_sum(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
        np.testing.assert_allclose(acc.cpu().numpy(), want, rtol=1e-12, atol=1e-12)
        acc = ops.channel_diff_sum(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), acc)   # accumulates
        np.testing.assert_allclose(acc.cpu().numpy(), 2 * want, rtol=1e-12, atol=1e-12)
    # an unaligned view (rows not starting on 16 bytes)
    flat = torch.from_numpy(rng.standard_normal(2 * 4 * 36 + 1).astype(np.float32)).to(dev)
    a = flat[1:].reshape(2, 4, 36)
    b = torch.zeros_like(a)
    np.testing.assert_allclose(ops.channel_diff_sum(a, b).cpu().numpy(), a.double().sum((0, 2)).cpu().numpy(), rtol=1e-12)


def test_octav_randomised_shapes_and_distributions(dev):
    """A seeded sweep over odd sizes (not multiples of 4, below / above the small-pair threshold, split over several
    workgroups) and distributions (discrete-valued, sparse, constant, huge / tiny scale, heavy tails): the three forms
    agree with each other and with the numpy oracle, for both `dynamic_sym` settings, in batched launches."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(20260)
    sizes = [1, 3, 17, 1023, 1025, 4099, 16383, 16385, 50001, 131071, 300003, 1200007]

    def draw(kind, n):
        if kind == 0:
            return rng.standard_normal(n) * 10 ** rng.uniform(-3, 3)
        if kind == 1:
            return np.maximum(rng.standard_normal(n) - rng.uniform(-1, 1), 0) * 10 ** rng.uniform(-2, 2)
        if kind == 2:
            return rng.integers(-8, 9, n) * 0.25                         # discrete values: many ties
        if kind == 3:
            return np.where(rng.random(n) < 0.02, rng.standard_normal(n) * 5, 0.0)
        if kind == 4:
            return np.full(n, rng.uniform(0.1, 3.0))                     # constant
        if kind == 5:
            return rng.standard_t(2.5, n)                                # heavy tails
        if kind == 6:
            return np.abs(rng.standard_normal(n)) + 1e-7                 # |min| < 1e-6: dynamic_sym trigger
        return rng.lognormal(0, 2.0, n) * rng.choice([-1, 1], n)
    B = 2
    elems, tensors, raw = [], [], []
    for t, n in enumerate(sizes):
        data = np.stack([draw((t + b) % 8, n) for b in range(B)]).astype(np.float32)
        raw.append(data)
        elems.append(n)
        tensors.append(torch.from_numpy(data).to(dev))
    plan = ops.TensorSetPlan(elems, B, dev)
    for dyn in (False, True):
        got = {form: _octav(ops, plan, tensors, dyn, form) for form in ("bracket", "compact", "full")}
        assert _same_steps(got["bracket"], got["compact"])
        assert _same_steps(got["bracket"], got["full"])
        for t, n in enumerate(sizes):
            for b in range(B):
                x = raw[t][b]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    s = O.octav_scale(x, O.octav_unsigned(x.min(), dyn))
                g = got["bracket"][b, t]
                assert _close(g[0], s), (n, b, dyn, g, s)
                assert g[1] == x.min() and g[2] == x.max()


@pytest.mark.parametrize("sets,lanes", [(3, 2), (2, 2), (4, 2), (3, 1), (3, 3), (2, 3)])
def test_octav_pipeline_matches_single_stream(dev, kl, monkeypatch, sets, lanes):
    """(sets: how many batches the host runs ahead = sets of per-batch scratch, ops._PIPE_SETS.  lanes: the streams the streaming
    kernels of consecutive batches rotate over — 2 by default: batch i + 1 starts while batch i drains; 1: the caller's stream.)
    OctavPipeline (rescue / walk of batch i on a side stream beside the streaming kernel of batch i + 1, rotating scratch)
    returns what the two-read form returns batch by batch — including the first batches, which run without any history — and
    the oracle's scales."""
    from dipoorlet_amd import ops
    monkeypatch.setenv("DPL_OCTAV_FORM", "tail")
    monkeypatch.setenv("DPL_OCTAV_LANES", str(lanes))
    monkeypatch.setattr(ops, "_PIPE_SETS", sets)
    rng = np.random.default_rng(41)
    B, sizes = 4, [401408, 30000, 802816, 777, 200704]
    batches = []
    for k in range(7):
        batches.append([torch.from_numpy(np.stack([
            ((rng.standard_normal(n) * (1 + 0.3 * k + t)).astype(np.float32) if t % 2 == 0 else
             np.maximum(rng.standard_normal(n), 0).astype(np.float32) * (2.5 + k)) for _ in range(B)])).to(dev)
            for t, n in enumerate(sizes)])
    want = [ops.octav_batch(ops.TensorSetPlan(sizes, B, dev), x, False, form="bracket").cpu().numpy() for x in batches]
    plan = ops.TensorSetPlan(sizes, B, dev)
    pipe = ops.OctavPipeline(False, dev)
    outs = [pipe.submit(plan, x) for x in batches]
    del batches                                   # the pipeline keeps what its side stream still reads
    pipe.sync()
    for k, (o, w) in enumerate(zip(outs, want)):
        got = o.cpu().numpy()
        assert np.array_equal(got[:, :, 1:], w[:, :, 1:]), k
        assert _close(got[:, :, 0], w[:, :, 0]), k      # (the two-read form walks the reference's iterates, the exact tail reaches their fixed point)
    # a second run on the same plan (threshold history warmed up), interleaved with a ragged plan
    plan2 = ops.TensorSetPlan(sizes, 2, dev)
    x = [torch.from_numpy(np.stack([(rng.standard_normal(n) * (1 + t)).astype(np.float32) for _ in range(B)])).to(dev)
         for t, n in enumerate(sizes)]
    a = pipe.submit(plan, x)
    b = pipe.submit(plan2, [v[:2].contiguous() for v in x])
    c = pipe.submit(plan, x)
    pipe.sync()
    assert np.array_equal(a.cpu().numpy()[..., 1:], c.cpu().numpy()[..., 1:]) and _close(a.cpu().numpy()[..., 0], c.cpu().numpy()[..., 0])
    assert _close(a.cpu().numpy()[:2, :, 0], b.cpu().numpy()[..., 0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for t in range(len(sizes)):
            assert _close(a[1, t, 0].item(), O.octav_scale(x[t][1].cpu().numpy(), 1))


def test_octav_special_values(dev, monkeypatch):
    """Values the histogram window (2^-18 .. 2^14) does not hold, and the ones IEEE sets apart: all zeros, signed zeros, NaN,
    +-inf, denormals, tiny normals below the window mixed into ordinary data, a pair that lies below the window entirely,
    values on the window's two edges, one huge outlier, a single non-zero — every form against the numpy oracle
    (forward_net.py:315-330 on such data: NaN and inf propagate through the sums, 0 / 0 is NaN), on one stream and through the
    pipeline."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(77)
    n = 70001

    def base():
        return rng.standard_normal(n).astype(np.float32) * 2

    def put(x, idx, v):
        x = x.copy()
        x[idx] = v
        return x
    some = rng.integers(0, n, 9)
    mk = [
        np.zeros(n, np.float32),                                                      # 0 / 0
        np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32),
        put(base(), some, np.nan),
        put(base(), some[:1], np.inf),
        put(base(), some[:2], -np.inf),
        put(np.maximum(base(), 0), some, np.float32(1e-40)),                           # denormals among ReLU outputs
        put(base(), some, np.float32(2.0 ** -30)),                                     # normals below the window (exact power of two)
        (rng.standard_normal(n) * 1e-7).astype(np.float32),                            # the whole pair below the window
        put(put(base(), some[:3], np.float32(2.0 ** -18)), some[3:6], np.float32(2.0 ** 14)),   # both edges
        put(base(), some[:1], np.float32(3e30)),                                       # one huge outlier
        put(np.zeros(n, np.float32), some[:1], np.float32(0.75)),                      # a single non-zero
        put(np.abs(base()), some, np.float32(1e-45)),                                  # smallest denormal; min >= 0: dynamic_sym
    ]
    B = 2
    tensors = [torch.from_numpy(np.stack([x, x[::-1].copy()])).to(dev) for x in mk]
    sizes = [n] * len(mk)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for dyn in (False, True):
            want = np.array([[O.octav_scale(t[b].cpu().numpy(), O.octav_unsigned(t[b].cpu().numpy().min(), dyn)) for t in tensors]
                             for b in range(B)], np.float64)
            plan = ops.TensorSetPlan(sizes, B, dev)
            got = {form: _octav(ops, plan, tensors, dyn, form) for form in ("bracket", "compact", "full")}
            got["tail"] = _octav(ops, ops.TensorSetPlan(sizes, B, dev), tensors, dyn, "tail")
            for form, g in got.items():
                for t in range(len(mk)):
                    for b in range(B):
                        assert _close(g[b, t, 0], want[b, t]), (form, dyn, t, b, g[b, t], want[b, t])
                        x = tensors[t][b].cpu().numpy()
                        if not np.isnan(x).any():
                            assert g[b, t, 1] == x.min() and g[b, t, 2] == x.max(), (form, t, b)
            monkeypatch.setenv("DPL_OCTAV_FORM", "tail")
            pipe = ops.OctavPipeline(dyn, dev)
            plan2 = ops.TensorSetPlan(sizes, B, dev)
            rows = [pipe.submit(plan2, tensors) for _ in range(3)]
            pipe.sync()
            for r in rows:
                assert np.array_equal(r.cpu().numpy()[..., 1:], got["tail"][..., 1:], equal_nan=True)
                assert _close(r.cpu().numpy()[..., 0], got["tail"][..., 0]), dyn
            monkeypatch.delenv("DPL_OCTAV_FORM")


def test_octav_tail_randomised_shapes_and_distributions(dev):
    """The exact-tail form over odd sizes (not multiples of 4, around the small-pair threshold, up to the one-slice cap) and
    distributions (discrete-valued, sparse, constant, huge / tiny scale, heavy tails, saturating, per-channel scales with the
    hot channels first / last): against the numpy oracle and the two-read form, both `dynamic_sym` settings, cold and warm."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(20264)
    sizes = [1, 3, 17, 1023, 1025, 4099, 16383, 20480, 20481, 50001, 131071, 300003, 605184, 1044480]

    def draw(kind, n):
        if kind == 0:
            return rng.standard_normal(n) * 10 ** rng.uniform(-3, 3)
        if kind == 1:
            return np.maximum(rng.standard_normal(n) - rng.uniform(-1, 1), 0) * 10 ** rng.uniform(-2, 2)
        if kind == 2:
            return rng.integers(-8, 9, n) * 0.25                         # discrete values: many ties
        if kind == 3:
            return np.where(rng.random(n) < 0.02, rng.standard_normal(n) * 5, 0.0)
        if kind == 4:
            return np.full(n, rng.uniform(0.1, 3.0))                     # constant
        if kind == 5:
            return rng.standard_t(2.5, n)                                # heavy tails
        if kind == 6:
            return np.abs(rng.standard_normal(n)) + 1e-7                 # |min| < 1e-6: dynamic_sym trigger
        if kind == 7:
            return np.clip(rng.standard_normal(n) * 3, 0, 6)             # saturating: an atom at the maximum
        if kind == 8:
            return rng.uniform(-1, 1, n)                                 # thin tail: the fixed point holds 0.3 % of the pair
        if kind == 9:                                                    # channel-major, the hot channels first / last
            c = 16
            sc = np.ones((c, 1))
            sc[:2 if rng.random() < 0.5 else -2] = 12.0
            return (rng.standard_normal((c, n // c + 1)) * sc).ravel()[:n]
        return rng.lognormal(0, 2.0, n) * rng.choice([-1, 1], n)
    B = 2
    elems, tensors, raw = [], [], []
    for t, n in enumerate(sizes):
        data = np.stack([draw((t + 3 * b) % 11, n) for b in range(B)]).astype(np.float32)
        raw.append(data)
        elems.append(n)
        tensors.append(torch.from_numpy(data).to(dev))
    plan = ops.TensorSetPlan(elems, B, dev)
    for dyn in (False, True):
        got = _octav(ops, plan, tensors, dyn, "tail")
        ref = ops.octav_batch(ops.TensorSetPlan(elems, B, dev), tensors, dyn, form="bracket").cpu().numpy()
        assert np.array_equal(got[..., 1:], ref[..., 1:]) and _close(got[..., 0], ref[..., 0])
        for t, n in enumerate(sizes):
            for b in range(B):
                x = raw[t][b]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    s = O.octav_scale(x, O.octav_unsigned(x.min(), dyn))
                g = got[b, t]
                assert _close(g[0], s), (n, b, dyn, g, s)
                assert g[1] == x.min() and g[2] == x.max()


WALK_EDGE_SIZES = [1279, 1280, 1281, 12287, 12288, 12289, 16384, 16385, 20480]


def _walk_edge_inputs():
    """-> (signed, unsigned): per size of WALK_EDGE_SIZES a [2, n] float32 array, |x| uniform in [0.05, 4) — every value non-zero
    and inside the histogram window — with random signs; `unsigned` is |x| with one element of every pair set to 1e-7 (below the
    window: |min| < 1e-6, what `dynamic_sym` looks for)."""
    rng = np.random.default_rng(12288)
    signed, unsigned = [], []
    for n in WALK_EDGE_SIZES:
        a = rng.uniform(0.05, 4.0, (2, n)).astype(np.float32)
        a = np.clip(a, np.float32(0.05), np.nextafter(np.float32(4.0), np.float32(0.0)))    # (the float32 rounding of the draw)
        signed.append(a * rng.choice(np.array([-1.0, 1.0], np.float32), (2, n)))
        u = a.copy()
        u[np.arange(2), rng.integers(0, n, 2)] = np.float32(1e-7)
        unsigned.append(u)
    return signed, unsigned


def test_octav_tail_list_lengths_at_the_walk_paths_edges(dev):
    """The exact-tail form with a list exactly as long as the sizes at which its walk takes another path: kFitCap = kSurvCap =
    1280 values (a list that one wave's registers hold; the staging area of the compaction through LDS) and kTailVec x 1024 =
    12288 (the rows resident in the workgroup's registers: beyond them kOver = 4 rows are streamed at a time) — one less, equal,
    one more; 16384 / 16385 (the first streamed group full / a second one begun) and kSmallCap = 20480.  A pair of at most
    kSmallCap elements lists its whole window, so a pair whose values are all non-zero and inside the window has a list as long
    as itself; with `dynamic_sym` one value per pair lies below the window (what makes the minimum count as zero) and the list
    is one shorter.  Cold and warm, against the numpy oracle; the control block says that exactly those values were listed and
    that no pair left for the rescue or the compaction route: the walks under test produced the results."""
    from dipoorlet_amd import _hip, ops
    B, sizes = 2, WALK_EDGE_SIZES
    signed, unsigned = _walk_edge_inputs()
    for dyn, raw in ((False, signed), (True, unsigned)):
        tensors = [torch.from_numpy(x).to(dev) for x in raw]
        want = np.array([[O.octav_scale(x[b], O.octav_unsigned(x[b].min(), dyn)) for x in raw] for b in range(B)], np.float64)
        assert np.isfinite(want).all()
        listed = sum(int(np.count_nonzero(np.abs(x) >= np.float32(2.0 ** -18))) for x in raw)
        assert listed == B * sum(sizes) - (B * len(sizes) if dyn else 0)
        plan = ops.TensorSetPlan(sizes, B, dev)
        states = torch.empty((plan.n_pairs + 1) * 80, dtype=torch.uint8, device=dev)
        for call in ("cold", "warm"):
            got = ops.octav_batch(plan, tensors, dyn, states, form="tail").cpu().numpy()
            ctl = _hip.OctavState.from_buffer_copy(states.cpu().numpy()[-80:].tobytes())
            assert ctl.sum == float(listed), (dyn, call, ctl.sum, listed)                   # every pair listed its whole window
            assert int(ctl.len0) == 0 and int(ctl.cnt_le) == 0, (dyn, call, int(ctl.len0), int(ctl.cnt_le))
            for t, n in enumerate(sizes):
                for b in range(B):
                    x = raw[t][b]
                    assert _close(got[b, t, 0], want[b, t]), (dyn, call, n, b, got[b, t], want[b, t])
                    assert got[b, t, 1] == x.min() and got[b, t, 2] == x.max(), (dyn, call, n, b)


def test_octav_tail_thresholds_follow_the_images(dev, monkeypatch):
    """What the exact-tail form lists and how often it has to be rescued, over a run of batches through the pipeline: images
    alike (thresholds from the earlier batches: ~1 % listed, next to no rescues), then images that differ in scale by +-30 %
    (a brighter image raises its threshold on the fly; a dimmer one may need the rescue) — results equal to the oracle's
    either way."""
    from dipoorlet_amd import ops
    monkeypatch.setenv("DPL_OCTAV_FORM", "tail")      # (the bounds below are this form's, whatever the environment selects)
    rng = np.random.default_rng(91)
    B, sizes = 4, [401408, 100352, 802816, 25088, 200704]
    plan = ops.TensorSetPlan(sizes, B, dev)
    for jitter in (0.0, 0.3):
        batches = []
        for k in range(6):
            f = 1.0 + jitter * (2.0 * rng.random((B, 1)) - 1.0)
            batches.append([torch.from_numpy((np.maximum(rng.standard_normal((B, n)), 0 if t % 2 else -1e30) * (1 + t) * f).astype(np.float32)).to(dev)
                            for t, n in enumerate(sizes)])
        plan.octav_reset()
        pipe = ops.OctavPipeline(False, dev)
        rows = [pipe.submit(plan, x) for x in batches]
        pipe.sync()
        assert pipe.batches == len(batches) and pipe.compaction_pairs == 0
        if jitter == 0.0:
            assert pipe.fallback_pairs <= 2 and pipe.list_share < 0.03, (pipe.fallback_pairs, pipe.list_share)
        else:
            assert pipe.fallback_pairs <= plan.n_pairs and pipe.max_share < 0.08, (pipe.fallback_pairs, pipe.max_share)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for k in (0, 5):
                got = rows[k].cpu().numpy()
                for t in range(len(sizes)):
                    for b in (0, B - 1):
                        x = batches[k][t][b].cpu().numpy()
                        assert _close(got[b, t, 0], O.octav_scale(x, 1)), (jitter, k, t, b)
                        assert got[b, t, 1] == x.min() and got[b, t, 2] == x.max()


def test_two_pipelines_share_a_plan(dev, monkeypatch):
    """An OctavPipeline owns its rotation state (scratch sets, state arrays, snapshots, call counter) per plan: two pipelines —
    calibration and profiling, or two threads — may run the same TensorSetPlan interleaved without corrupting each other
    (re-entrant ops, no hidden mutable state on the plan)."""
    from dipoorlet_amd import ops
    monkeypatch.setenv("DPL_OCTAV_FORM", "tail")
    rng = np.random.default_rng(77)
    B, sizes = 2, [200704, 30000, 802816]
    plan = ops.TensorSetPlan(sizes, B, dev)
    batches = [[torch.from_numpy((rng.standard_normal((B, n)) * (1 + t + 0.2 * k)).astype(np.float32)).to(dev) for t, n in enumerate(sizes)]
               for k in range(8)]
    p1, p2 = ops.OctavPipeline(False, dev), ops.OctavPipeline(False, dev)
    r1, r2 = [], []
    for k, x in enumerate(batches):          # p2 runs the batches in reverse order, interleaved with p1
        r1.append(p1.submit(plan, x))
        r2.append(p2.submit(plan, batches[len(batches) - 1 - k]))
    p1.sync()
    p2.sync()
    torch.cuda.synchronize()
    want = [ops.octav_batch(ops.TensorSetPlan(sizes, B, dev), x, False, form="bracket").cpu().numpy() for x in batches]
    for k in range(len(batches)):
        for got in (r1[k].cpu().numpy(), r2[len(batches) - 1 - k].cpu().numpy()):
            assert np.array_equal(got[..., 1:], want[k][..., 1:]), k
            assert _close(got[..., 0], want[k][..., 0]), k


@pytest.mark.parametrize("lanes", [1, 2])
def test_pipeline_survives_octav_reset(dev, monkeypatch, lanes):
    """One pipeline reused across TensorSetPlan.octav_reset() — what every timed sweep of the benchmark does: the reset is
    refused while batches are in flight and leaves them to finish with the right rows; after sync() it zeroes the threshold
    history, the rotation starts over, and the same batches give the same rows again (a small pair, a one-slice pair and a
    whole-window pair; five batches: more than S + 1, so every set is reused on both sides of the reset)."""
    from dipoorlet_amd import _hip, ops
    monkeypatch.setenv("DPL_OCTAV_FORM", "tail")
    rng = np.random.default_rng(79)
    B, sizes = 2, [30000, 200704, 777]
    batches = [[torch.from_numpy((rng.standard_normal((B, n)) * (1 + t + 0.2 * k)).astype(np.float32)).to(dev) for t, n in enumerate(sizes)]
               for k in range(5)]
    want = [ops.octav_batch(ops.TensorSetPlan(sizes, B, dev), x, False, form="bracket").cpu().numpy() for x in batches]

    def same_rows(rows):
        for k, (o, w) in enumerate(zip(rows, want)):
            got = o.cpu().numpy()
            assert np.array_equal(got[..., 1:], w[..., 1:]), k
            assert _close(got[..., 0], w[..., 0]), k
    plan = ops.TensorSetPlan(sizes, B, dev)
    pipe = ops.OctavPipeline(False, dev, lanes=lanes)
    pipe.record_events = True
    rows = [pipe.submit(plan, x) for x in batches]
    with pytest.raises(_hip.DipoorletHipError):
        plan.octav_reset()                          # batches in flight
    pipe.sync()
    torch.cuda.synchronize()
    same_rows(rows)
    assert pipe.batches == 5 and len(pipe.events) == 5
    assert all(began.elapsed_time(streamed) > 0 for began, streamed in pipe.events)
    plan.octav_reset()
    pipe.reset_stats()
    assert not plan.octav_tail().history.any().item()
    rows = [pipe.submit(plan, x) for x in batches]
    pipe.sync()
    same_rows(rows)
    assert pipe.batches == 5 and pipe.compaction_pairs == 0


@pytest.mark.parametrize("hook", ["exact", "rescue"])
def test_two_pipelines_rescue_at_once(dev, monkeypatch, hook):
    """Two pipelines on ONE plan whose walks are refused for every second pair (the C ABI's test hooks) rescue the same pair
    indices of different batches at the same time, each on its own side stream: every pipeline owns its rescue list, rescue rows
    and — `rescue`: the rescue walk is refused too — the compaction route's lists (a plan-level rescue list let one
    pipeline's gather overwrite the other's)."""
    from dipoorlet_amd import _hip, ops
    monkeypatch.setenv("DPL_OCTAV_FORM", "tail")
    rng = np.random.default_rng(78)
    B, sizes = 2, [200704, 30000, 802816, 401408]
    plan = ops.TensorSetPlan(sizes, B, dev)
    batches = [[torch.from_numpy((rng.standard_normal((B, n)) * (1 + t + 0.5 * k)).astype(np.float32)).to(dev) for t, n in enumerate(sizes)]
               for k in range(8)]
    want = [ops.octav_batch(ops.TensorSetPlan(sizes, B, dev), x, False, form="bracket").cpu().numpy() for x in batches]
    L = _hip.lib()
    old = (L.dpl_test_hook_exact_fail_every(2), L.dpl_test_hook_rescue_fail_every(2 if hook == "rescue" else 0))
    try:
        p1, p2 = ops.OctavPipeline(False, dev), ops.OctavPipeline(False, dev)
        r1, r2 = [], []
        for k, x in enumerate(batches):
            r1.append(p1.submit(plan, x))
            r2.append(p2.submit(plan, batches[len(batches) - 1 - k]))
        p1.sync()
        p2.sync()
        torch.cuda.synchronize()
    finally:
        L.dpl_test_hook_exact_fail_every(old[0])
        L.dpl_test_hook_rescue_fail_every(old[1])
    assert p1.fallback_pairs >= len(batches) * plan.n_pairs // 4 and p2.fallback_pairs >= len(batches) * plan.n_pairs // 4
    if hook == "rescue":
        assert p1.compaction_pairs > 0 and p2.compaction_pairs > 0
    for k in range(len(batches)):
        for got in (r1[k].cpu().numpy(), r2[len(batches) - 1 - k].cpu().numpy()):
            assert np.array_equal(got[..., 1:], want[k][..., 1:]), k
            assert _close(got[..., 0], want[k][..., 0]), k


def test_octav_tail_lists_beyond_their_regions(dev, monkeypatch):
    """The exact-tail form's list regions hold dpl_octav_list_cap(n) values per pair (n / 16 + 16384), not the pair: what a pair
    lists — or its rescue gathers — beyond that is dropped and the pair finishes on the compaction route, whose whole-batch
    lists the pipeline allocates only when a batch first asks for them.  Saturating activations (a third of the values AT the
    maximum: every one of them is above any threshold), a constant tensor, a two-level one and a dense small pair next to
    ordinary tensors; the scratch of the pipeline stays below half the batch's activations until then."""
    from dipoorlet_amd import _hip, ops
    monkeypatch.setenv("DPL_OCTAV_FORM", "tail")
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    B = 4
    sizes = [802816, 401408, 20480, 602112, 300000, 150528]
    kinds = ["normal", "saturated", "dense_small", "const", "two_level", "relu"]

    def draw(kind, n, scale):
        z = torch.randn(B, n, generator=g, device=dev) * scale
        if kind == "saturated":
            z = z.clamp_(-0.4 * scale, 0.4 * scale)            # ~ 2/3 of a normal's mass sits on the two rails
        elif kind == "dense_small":
            z = z.abs_() + 0.5                                 # no zeros: the small pair lists all 20 480 values
        elif kind == "const":
            z = torch.full((B, n), 1.25 * scale, device=dev)
        elif kind == "two_level":
            z = torch.where(z > 0, torch.full_like(z, 2.0 * scale), torch.full_like(z, 0.125))
        elif kind == "relu":
            z = z.clamp_(min=0)
        return z.contiguous()
    batches = [[draw(k, n, 1.0 + 0.3 * it) for k, n in zip(kinds, sizes)] for it in range(6)]
    want = [ops.octav_batch(ops.TensorSetPlan(sizes, B, dev), x, False, form="bracket").cpu().numpy() for x in batches]
    plan = ops.TensorSetPlan(sizes, B, dev)
    pipe = ops.OctavPipeline(False, dev)
    outs = [pipe.submit(plan, batches[0])]
    before = pipe.scratch_bytes(plan)
    assert before < 0.5 * 4 * B * sum(sizes)
    assert _hip.lib().dpl_octav_list_cap(401408) < 401408 // 4      # (the saturated pair's ~270 k rail values cannot fit)
    outs += [pipe.submit(plan, x) for x in batches[1:]]
    pipe.sync()
    torch.cuda.synchronize()
    # the constant tensor in every image of every batch; the saturated / two-level ones whenever their rail is not a bin edge (an
    # iterate just below a power of two sits in the EMPTY bin under the rail's: the rescue then needs no values at all)
    assert pipe.compaction_pairs >= 2 * B * len(batches)
    # ... and the compaction route's lists exist now: regions for just the pairs that took the route (dpl_octav_fallback_layout)
    after = pipe.scratch_bytes(plan)
    assert before + 2 * 4 * B * sizes[3] <= after <= before + 3.1 * 4 * B * (sizes[1] + sizes[3] + sizes[4]) + 65536
    for k, (o, w) in enumerate(zip(outs, want)):
        got = o.cpu().numpy()
        assert np.array_equal(got[..., 1:], w[..., 1:]), k
        assert _close(got[..., 0], w[..., 0]), (k, got[..., 0], w[..., 0])
    single = ops.octav_batch(ops.TensorSetPlan(sizes, B, dev), batches[2], False).cpu().numpy()      # one stream, cold
    assert np.array_equal(single[..., 1:], want[2][..., 1:]) and _close(single[..., 0], want[2][..., 0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for t in (1, 2, 3, 4):
            assert _close(single[0, t, 0], O.octav_scale(batches[2][t][0].cpu().numpy(), 1)), t


def test_fake_quant_set_launch_matches_per_tensor_launches(dev):
    """dpl_fake_quant_items — a whole tensor set fake-quantised in ONE launch — against one dpl_fake_quant launch per tensor and
    the oracle (ONNX opset-13 Q -> DQ, quantize.py:197-239), bit for bit: per-tensor and per-channel rows mixed, channel rows
    that are / are not a multiple of four long (7 x 7 maps take the element-wise path), sizes that are no multiple of 1024 (a
    workgroup's share ends inside a vector), uint8 and int8 grids with non-zero zero points, in place and out of place."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(61)
    B = 3
    shapes = [(16, 14, 14), (8, 7, 7), (5, 33, 3), (64, 56, 56), (1, 1000, 1), (12, 4, 4), (3, 224, 224)]
    elems = [c * h * w for c, h, w in shapes]
    plan = ops.TensorSetPlan(elems, B, dev)
    xs, params, want = [], [], []
    for t, (c, h, w) in enumerate(shapes):
        x = (rng.standard_normal((B, c, h, w)) * (1 + t)).astype(np.float32)
        per_channel = t % 2 == 0
        signed = t % 3 != 0
        qlo, qhi = (-128, 127) if signed else (0, 255)
        nch = c if per_channel else 1
        scale = (np.abs(rng.standard_normal(nch)) * 0.05 + 0.01).astype(np.float32)
        zp = rng.integers(-5, 6, nch).astype(np.int32) if signed else rng.integers(0, 256, nch).astype(np.int32)
        xs.append(torch.from_numpy(x).to(dev).reshape(B, -1))
        params.append((torch.from_numpy(scale), torch.from_numpy(zp), h * w, qlo, qhi))
        want.append(O.fake_quant_qdq(x, scale, zp, axis=1 if per_channel else None, signed=signed).reshape(B, -1))
    fset = ops.FakeQuantSet(plan, params)
    ys = fset(xs)
    for t, (c, h, w) in enumerate(shapes):
        sc, zp, inner, qlo, qhi = params[t]
        one = ops.fake_quant(xs[t].view(B, c, h * w), sc, zp, qlo, qhi, axis=1 if sc.numel() > 1 else None)
        assert np.array_equal(ys[t].cpu().numpy(), want[t]), t
        assert np.array_equal(one.reshape(B, -1).cpu().numpy(), want[t]), t
    again = [x.clone() for x in xs]
    fset(again, out=again)                       # in place
    for t in range(len(shapes)):
        assert np.array_equal(again[t].cpu().numpy(), want[t]), t


@pytest.mark.parametrize("fail_every", [0, 2])
def test_octav_tail_pairs_above_one_slice(dev, monkeypatch, fail_every):
    """The exact-tail form on pairs of MORE than one slice (> 1 044 480 elements per image and tensor: k_octav_tail's slice
    path + k_octav_tail_merge) next to ordinary ones: every route — accepted walks, the rescue (forced by the C ABI's test hook for every
    second pair), a bin of 2^20 values or more (a constant tensor: the merged packed words do not hold it, compaction route),
    values >= 2^14, NaN, an all-zero tensor, dynamic_sym — through the pipeline over batches that differ in scale, against the
    two-read form and the numpy oracle."""
    from dipoorlet_amd import _hip, ops
    monkeypatch.setenv("DPL_OCTAV_FORM", "tail")
    rng = np.random.default_rng(31)
    g = torch.Generator(device=dev)
    g.manual_seed(31)
    B = 2
    sizes = [1200007, 777, 3000000, 150528, 2097152, 1044481, 2500000, 1100003, 1300000]
    kinds = ["normal", "relu", "uniform", "normal", "const", "heavy", "huge", "nan", "zero"]

    def draw(kind, n, scale):
        z = torch.randn(B, n, generator=g, device=dev)
        if kind == "relu":
            z = z.clamp_(min=0)
        elif kind == "uniform":
            z = torch.rand(B, n, generator=g, device=dev) * 2 - 1
        elif kind == "const":
            z = torch.full((B, n), 0.37, device=dev)
        elif kind == "heavy":
            z = z * torch.exp(torch.randn(B, n, generator=g, device=dev))
        elif kind == "huge":
            z = z * 9000.0                      # values >= 2^14
        elif kind == "nan":
            z[0, n // 2] = float("nan")         # image 0 only
        elif kind == "zero":
            z = torch.zeros(B, n, device=dev)
        return (z * scale).contiguous()
    batches = [[draw(k, n, 1.0 + 0.25 * it + 0.1 * t) for t, (k, n) in enumerate(zip(kinds, sizes))] for it in range(4)]
    for dyn in (False, True):
        want = [ops.octav_batch(ops.TensorSetPlan(sizes, B, dev), x, dyn, form="bracket").cpu().numpy() for x in batches]
        old = _hip.lib().dpl_test_hook_exact_fail_every(fail_every)
        try:
            plan = ops.TensorSetPlan(sizes, B, dev)
            assert plan.octav_tail().n_multi == 7 * B
            pipe = ops.OctavPipeline(dyn, dev)
            outs = [pipe.submit(plan, x) for x in batches]
            pipe.sync()
            torch.cuda.synchronize()
            single = ops.octav_batch(ops.TensorSetPlan(sizes, B, dev), batches[1], dyn).cpu().numpy()    # (cold, one stream)
        finally:
            _hip.lib().dpl_test_hook_exact_fail_every(old)
        assert pipe.compaction_pairs >= 2 * B * len(batches)        # the constant tensor and the one beyond 2^14, every batch
        if fail_every:
            assert pipe.fallback_pairs >= len(batches) * plan.n_pairs // 4
        for k, (o, w) in enumerate(zip(outs + [single], want + [want[1]])):
            got = o.cpu().numpy() if hasattr(o, "cpu") else o
            assert np.array_equal(got[..., 1:], w[..., 1:], equal_nan=True), k
            assert _close(got[..., 0], w[..., 0]), (k, got[..., 0], w[..., 0])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = outs[-1].cpu().numpy()
            for t in (0, 2, 4, 5, 6, 7):
                for b in range(B):
                    x = batches[-1][t][b].cpu().numpy()
                    assert _close(got[b, t, 0], O.octav_scale(x, 4 if (dyn and abs(float(np.nanmin(x))) < 1e-6 and not np.isnan(x).any()) else 1)), (t, b)


def test_octav_tail_soak_short():
    """scripts/tail_soak.py for a few seconds: random tensor sets (sizes 1 .. 1 044 480, 16 distribution kinds, per-image scales up
    to x 4, both dynamic_sym settings) through the pipeline in the exact-tail form — threshold history, raises on the fly, rescues,
    the compaction route — every pair against the two-read form, a sample against the numpy oracle.  (The long runs:
    profiles/r04/tail_soak.txt — 4 M pairs, 0 mismatches.)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "tail_soak.py"), "8", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert " 0 mismatches" in r.stdout


def test_seg_table_checks_every_unbound_call(dev):
    """TensorSetPlan.seg_table: PyTorch's caching allocator hands a freed set's addresses to the next tensors, so a pointer tuple
    seen before proves nothing about the tensors behind it — an unbound tensor list is validated on EVERY launch
    (element count, dtype, contiguity, device); a set that is launched over again and again is bound once (TensorSetPlan.bind)
    and then held, which is what makes skipping the checks safe."""
    from dipoorlet_amd import _hip, ops
    sizes = [4096, 1000, 65536]
    B = 4
    plan = ops.TensorSetPlan(sizes, B, dev)
    acc = ops.CalibAccumulators(len(sizes), dev)
    xs = [torch.randn(B, n, device=dev) for n in sizes]
    acc.minmax_accumulate(plan, xs)                      # (the pointer tuple is cached now)
    ptrs = [x.data_ptr() for x in xs]
    del xs
    # the same addresses, fewer elements: tensors of half the batch in the blocks the allocator has just got back
    ys = [torch.randn(B // 2, n, device=dev) for n in sizes]
    if [y.data_ptr() for y in ys] != ptrs:               # (the allocator answered otherwise: views of one buffer give the same addresses)
        big = [torch.randn(B, n, device=dev) for n in sizes]
        acc.minmax_accumulate(plan, big)
        ys = [x[:B // 2] for x in big]
        assert [y.data_ptr() for y in ys] == [x.data_ptr() for x in big]
    with pytest.raises(_hip.DipoorletHipError, match="elements"):
        acc.minmax_accumulate(plan, ys)
    with pytest.raises(_hip.DipoorletHipError, match="contiguous float32"):
        acc.minmax_accumulate(plan, [torch.zeros(B, n, device=dev, dtype=torch.float16) for n in sizes])
    with pytest.raises(_hip.DipoorletHipError):
        plan.bind(ys)
    good = [torch.randn(B, n, device=dev) for n in sizes]
    bound = plan.bind(good)
    del good                                             # the BoundSet holds the tensors: their memory cannot be handed out again
    other = [torch.randn(B, n, device=dev) for n in sizes]
    assert not set(x.data_ptr() for x in other) & set(x.data_ptr() for x in bound)
    acc.minmax_accumulate(plan, bound)
    with pytest.raises(_hip.DipoorletHipError, match="another plan"):
        acc.minmax_accumulate(ops.TensorSetPlan(sizes, B, dev), bound)


def test_pipeline_streams_run_beside_the_callers_stream(dev):
    """OctavPipeline's side stream (and lanes) must run BESIDE the caller's stream: a normal-priority stream that shares its
    hardware queue runs behind it instead (ops._separate_stream asks the device; ops._runs_beside is the question).  A stream
    is never beside itself; the pipeline's choices are beside the caller's stream and beside each other.  dpl_stream_create makes
    the stream torch cannot (a low-priority one) and the range is gfx950's."""
    import ctypes as C

    from dipoorlet_amd import _hip, ops
    main = torch.cuda.current_stream(dev)
    s = torch.cuda.Stream(dev)
    assert ops._behind(dev, s, [s]) > 0.9 and ops._runs_beside(dev, s, [s]) is False
    pool = [torch.cuda.Stream(dev) for _ in range(8)]
    floor = min(ops._behind(dev, x, [main]) for x in pool)      # what "beside the caller's stream" reads on this box (separate
    for lanes in (1, 2):                                          # queues: 0.01 - 0.03; a shared one: 1.0)
        p = ops.OctavPipeline(False, dev, lanes=lanes)
        streams = [p.side] + p.lanes
        assert len(p.lanes) == (2 if lanes == 2 else 0)
        for x in streams:
            # (the answer is a timing on the device: a stream that shares a queue is behind EVERY time, one that does not may look
            # so once when something else delays its marker — asked up to three times)
            assert min(ops._behind(dev, x, [main]) for _ in range(3)) <= floor + 0.2, (lanes, floor)
            for y in streams:
                if y is not x:
                    assert min(ops._behind(dev, x, [y]) for _ in range(3)) < 0.5, lanes
    lo, hi = C.c_int(), C.c_int()
    _hip.check(_hip.lib().dpl_stream_priority_range(C.byref(lo), C.byref(hi)), "dpl_stream_priority_range")
    assert (lo.value, hi.value) == (1, -1)
    h = C.c_void_p()
    _hip.check(_hip.lib().dpl_stream_create(5, C.byref(h)), "dpl_stream_create")       # (clamped to the least urgent)
    ext = torch.cuda.ExternalStream(h.value, dev)
    with torch.cuda.stream(ext):
        y = torch.arange(8, device=dev).float().sum()
    ext.synchronize()
    assert float(y) == 28.0
    _hip.check(_hip.lib().dpl_stream_destroy(h), "dpl_stream_destroy")


# ------------------------------------------------------------------ the side kernels at their edges, against fp64 / numpy
def _same_f32(got, want):
    """fp32 bit for bit, except that any NaN equals any NaN (the kernel writes the canonical quiet NaN, numpy returns the one it
    met) and -0.0 equals +0.0: fminf / fmaxf may return either zero of a (-0, +0) pair, and so may numpy's vectorised min / max
    (the reference's np.min over a row of ±0 is a zero of either sign, the same number)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    same_bits = got.view(np.uint32) == want.view(np.uint32)
    return same_bits | (np.isnan(got) & np.isnan(want)) | ((got == 0) & (want == 0))


def test_rowwise_minmax_vs_numpy_rows_off_16_bytes(dev):
    """k_rowwise_minmax (every per-channel weight range, weight_clip_val.json) against the reference's np.min / np.max over
    tensor.reshape(c, -1) (basic_algorithm.py:72-91).  cols % 4 != 0 puts row r's start at byte 4 r cols, off 16 B: the scalar
    head and tail of stream_span; each row's extreme sits at its first element, its last, or one past its first 16-B boundary.
    Then NaN in ONE row (its neighbours stay finite), ±inf, all-equal rows, denormals, ±0, and the `out=` slices at an odd
    offset that find_clip_val_minmax_weight writes through."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(71)
    for cols in (1, 2, 3, 5, 9, 49, 63, 64, 65, 255, 257, 4097):
        for rows in (1, 3, 64, 1000):
            w = rng.standard_normal((rows, cols)).astype(np.float32)
            r = np.arange(rows)
            head = (-r * cols) % 4              # elements of row r in front of its first 16-B boundary (the buffer is aligned)
            at = [np.zeros(rows, np.int64), np.full(rows, cols - 1), np.minimum(head + 1, cols - 1)]
            w[r, np.choose(r % 3, at)] = np.float32(8) + r.astype(np.float32)
            w[r, np.choose((r + 1) % 3, at)] = np.float32(-8) - r.astype(np.float32)    # (cols < 3: the same element)
            lo, hi = ops.rowwise_minmax(torch.from_numpy(w).to(dev))
            assert _same_f32(lo.cpu().numpy(), w.min(1)).all(), (rows, cols)
            assert _same_f32(hi.cpu().numpy(), w.max(1)).all(), (rows, cols)
    # special values, one kind per row, on rows of 49 (every start off 16 B but the first) and of 1 (a bias, a BN vector)
    den = np.float32(1e-40)
    for cols in (49, 1):
        w = rng.standard_normal((12, cols)).astype(np.float32)
        w[1, cols // 2] = np.nan                                 # NaN: this row only
        w[3, -1] = np.inf
        w[4, 0] = -np.inf
        w[5, :] = np.float32(1.5)                                # all equal
        w[6, :] = den * rng.integers(-5, 6, cols).astype(np.float32)   # denormals
        w[7, :] = np.where(rng.integers(0, 2, cols) == 0, np.float32(-0.0), np.float32(0.0))
        w[8, 0], w[8, -1] = np.inf, -np.inf
        w[9, 0] = np.inf
        w[9, -1] = np.nan                                        # NaN beside inf: NaN
        w[10, :] = np.float32(-0.0)
        w[11, :] = -den
        lo, hi = ops.rowwise_minmax(torch.from_numpy(w).to(dev))
        lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
        assert _same_f32(lo, w.min(1)).all() and _same_f32(hi, w.max(1)).all(), (cols, lo, hi)
        assert np.isnan(lo[[1, 9]]).all() and np.isnan(hi[[1, 9]]).all()
        assert not np.isnan(np.delete(lo, [1, 9])).any() and not np.isnan(np.delete(hi, [1, 9])).any()
    # through out= slices of one result buffer at an odd offset; the values around the slices stay
    w = rng.standard_normal((37, 9)).astype(np.float32)
    res = torch.full((2, 45), 7.0, dtype=torch.float32, device=dev)
    off = 5
    ops.rowwise_minmax(torch.from_numpy(w).to(dev), out=(res[0, off:off + 37], res[1, off:off + 37]))
    got = res.cpu().numpy()
    assert _same_f32(got[0, off:off + 37], w.min(1)).all() and _same_f32(got[1, off:off + 37], w.max(1)).all()
    assert (np.delete(got, np.s_[off:off + 37], axis=1) == 7.0).all()


def _weight_graph():
    """Depthwise Conv (rows of 9) -> BatchNormalization -> PRelu (slope [C, 1, 1]) -> ConvTranspose (weight [C_in, C_out, 3, 3],
    ranged on its [1, 0, 2, 3] view) -> GlobalAveragePool -> Flatten -> Gemm (transB = 1): every kind of initializer
    find_clip_val_minmax_weight ranges."""
    from dipoorlet_amd.models import _B
    g = _B(83)
    x = g.conv("input", 8, 8, 3, 1, 1, "dw", groups=8)
    x = g.node("BatchNormalization", [x, g.b("bn.scale", 8, 1.0), g.b("bn.bias", 8), g.b("bn.mean", 8),
                                      g.const("bn.var", np.abs(g.rng.standard_normal(8)).astype(np.float32) + 0.5)],
               out="bn_out", epsilon=1e-5)
    x = g.node("PRelu", [x, g.const("prelu.slope", (g.rng.standard_normal((8, 1, 1)) * 0.1).astype(np.float32))], out="prelu_out")
    x = g.node("ConvTranspose", [x, g.w("ct.weight", (8, 5, 3, 3)), g.b("ct.bias", 5)], out="ct_out", kernel_shape=[3, 3],
               pads=[1, 1, 1, 1], strides=[1, 1], dilations=[1, 1], group=1)
    x = g.node("GlobalAveragePool", [x], out="gap_out")
    x = g.node("Flatten", [x], out="flat_out", axis=1)
    x = g.node("Gemm", [x, g.w("fc.weight", (10, 5)), g.b("fc.bias", 10)], out="fc_out", alpha=1.0, beta=1.0, transB=1)
    return g.finish("input", [1, 8, 10, 10], x)


def test_weight_ranges_of_a_graph_with_and_without_resident_constants(dev):
    """find_clip_val_minmax_weight (basic_algorithm.py:72-91) over a depthwise Conv, BN parameters, a PRelu slope, a
    ConvTranspose (the [1, 0, 2, 3] view) and a Gemm — with a session whose constants are resident (views of one device
    buffer) and without one (each initializer uploaded) — equals the reference's numpy, bit for bit."""
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.tensor_cali.basic_algorithm import find_clip_val_minmax_weight
    g = _weight_graph()
    want = {}
    for node in g.graph.node:
        if node.op_type not in ("Conv", "Gemm", "ConvTranspose", "PRelu", "BatchNormalization"):
            continue
        for name in list(node.input)[1:]:
            t = np.asarray(g.get_initializer(name))
            if t.ndim < 1:
                continue
            if node.op_type == "ConvTranspose" and name == node.input[1]:
                t = t.transpose([1, 0, 2, 3])
            want[name] = [np.min(t.reshape((t.shape[0], -1)), -1), np.max(t.reshape((t.shape[0], -1)), -1)]
    assert len(want) == 11 and want["ct.weight"][0].shape == (5,) and want["dw.weight"][0].shape == (8,)
    for session in (None, GraphSession(g, device=dev)):
        got = find_clip_val_minmax_weight(g, None, session=session)
        assert sorted(got) == sorted(want)
        for name, (lo, hi) in want.items():
            assert got[name][0].shape == lo.shape and got[name][1].shape == hi.shape, name
            assert _same_f32(got[name][0], lo).all() and _same_f32(got[name][1], hi).all(), (name, session is None)


def _cos_sums(a, b):
    """(Σab, Σaa, Σbb) per row in fp64 (products of two fp32 values are exact in fp64): utils.py:273-278's partial sums."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.stack([(a * b).sum(-1), (a * a).sum(-1), (b * b).sum(-1)], -1)


def test_cos_per_image_vs_fp64_unaligned_segments(dev):
    """k_cos_items (--profiling's per-layer cosine, profiling.py:74) against fp64 numpy per (image, tensor): per-image segments
    of 1, 3, 5, 1023 ... elements start off 16 B (the scalar path), 802816-element tensors are cut into several work items, a
    zero tensor (Σaa = 0), a == b (Σab is the same sum as Σaa), magnitudes around 1e18 (fp64 squares are finite where fp32
    sums would overflow).  Balanced items and one item of 1024 elements per workgroup (an item of an unaligned segment starts
    off 16 B as the segment does)."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(73)
    sizes = [1, 3, 4, 5, 1023, 1025, 4097, 50001, 802816]
    for B in (1, 3, 5):
        a = [rng.standard_normal((B, e)).astype(np.float32) for e in sizes]
        b = [(np.float32(0.9) * x + np.float32(0.3) * rng.standard_normal(x.shape).astype(np.float32)).astype(np.float32) for x in a]
        a[4][:] = 0                                   # a zero tensor
        b[2], b[5] = a[2].copy(), a[5].copy()         # a == b
        a[6] *= np.float32(1e18)                      # a*a, b*b around 1e36: finite in fp64
        b[6] *= np.float32(3e18)
        ta = [torch.from_numpy(x).to(dev) for x in a]
        tb = [torch.from_numpy(x).to(dev) for x in b]
        for chunk in (None, 1024):
            plan = ops.TensorSetPlan(sizes, B, dev, chunk_elems=chunk)
            got = ops.cos_per_image(plan, ta, tb).cpu().numpy()
            assert got.shape == (B, len(sizes), 3)
            for t in range(len(sizes)):
                np.testing.assert_allclose(got[:, t], _cos_sums(a[t], b[t]), rtol=1e-12, atol=0, err_msg=f"B={B} t={t} {chunk}")
            assert (got[:, 4, :2] == 0).all()               # (Σab = Σaa = 0 exactly)
            assert np.array_equal(got[:, 2, 0], got[:, 2, 1]) and np.array_equal(got[:, 5, 0], got[:, 5, 2])


def test_cos_accumulate_slots_tails_and_refusals(dev):
    """k_cos_acc (utils.py:273-278 partial sums into acc[slot]) against fp64 numpy: slot > 0, two accumulations into the same
    slot, n % 4 in {1, 2, 3}, the other slots untouched.  A buffer off 16 B, an accumulator of the wrong type or one without
    the slot are refused on the host before any launch, and the accumulator keeps its values."""
    from dipoorlet_amd import _hip, ops
    rng = np.random.default_rng(75)
    acc = torch.zeros(4, 3, dtype=torch.float64, device=dev)
    for n in (1, 2, 3, 5, 4097, 123458, 1000003):
        acc.zero_()
        pairs = [(rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)) for _ in range(2)]
        pairs[0] = (pairs[0][0], pairs[0][0] * np.float32(0.9) + pairs[0][1] * np.float32(0.3))
        pairs[1] = (pairs[1][0] * np.float32(1e18), pairs[1][0] * np.float32(7e17) + pairs[1][1] * np.float32(1e17))
        for a, b in pairs:
            ops.cos_accumulate(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), acc, slot=2)
        got = acc.cpu().numpy()
        want = _cos_sums(*pairs[0]) + _cos_sums(*pairs[1])
        np.testing.assert_allclose(got[2], want, rtol=1e-12, atol=0, err_msg=str(n))
        assert (np.delete(got, 2, axis=0) == 0).all(), n
    before = acc.clone()
    buf = torch.ones(1026, device=dev)
    with pytest.raises(_hip.DipoorletHipError):
        ops.cos_accumulate(buf[1:1025], buf[:1024], acc, slot=1)          # 4 B off 16
    with pytest.raises(_hip.DipoorletHipError):
        ops.cos_accumulate(buf[:1024], buf[2:1026], acc, slot=1)          # 8 B off 16
    with pytest.raises(_hip.DipoorletHipError):
        ops.cos_accumulate(buf[:1024], buf[:1024], acc, slot=4)           # no slot 4 in a [4, 3] accumulator
    with pytest.raises(_hip.DipoorletHipError):
        ops.cos_accumulate(buf[:1024], buf[:1024], acc.float(), slot=0)   # fp32: the kernel adds fp64
    assert torch.equal(acc, before)


def _percentile_cases(bins, rng):
    """(hist, gmin, gmax) of constructed histograms for `bins` bins, and the thresholds to ask: power-of-two totals whose
    cumulative sum reaches 0.5 / 0.75 EXACTLY at the end of bin 0, 63, 64 or bins - 1 (1.0 there), random counts above 2^24
    (fl32(count) rounds), an all-zero histogram; ranges symmetric and not, so that max(-clip, gmin) and min(clip, gmax) pick
    either side."""
    ranges = [(-1.0, 1.0), (-0.25, 3.0), (-5.0, 0.5), (0.0, 2.0), (-2.0, -0.5), (-1e-3, 1e-3)]
    cases, thrs = [], {0.5, 0.75, 1.0, 0.99999, 0.999, 1.5}
    total = 1 << 20
    for target in sorted({0, 63, 64, bins - 1}):
        if target >= bins:
            continue
        for thr in ((1.0,) if target == bins - 1 else (0.5, 0.75)):
            need = int(thr * total)
            h = np.zeros(bins, np.int64)
            h[target] = need if target == 0 else need // 3 + 1
            if target:
                h[:target] += rng.multinomial(need - h[target], np.full(target, 1.0 / target))
            if need < total:
                h[target + 1:] += rng.multinomial(total - need, np.full(bins - target - 1, 1.0 / (bins - target - 1)))
            assert h.sum() == total and h[:target + 1].sum() == need
            cases.append(h)
    for scale in (1 << 26, 1 << 40):                 # above 2^24: fl32(count) is not count
        h = rng.integers(0, scale, bins).astype(np.int64)
        h[rng.integers(0, bins, bins // 3)] = 0
        cases.append(h)
    cases.append(np.zeros(bins, np.int64))           # never reached: [gmin, gmax]
    out = [(h, *ranges[i % len(ranges)]) for i, h in enumerate(cases)]
    return out, sorted(thrs)


def test_hist_percentile_constructed_histograms_vs_oracle(dev):
    """k_hist_percentile (every -A hist clip, basic_algorithm.py:40-53) bit for bit against O.hist_percentile on histograms
    built here rather than taken from k_abs_hist: the threshold met exactly on a bin boundary, in bin 0, at bins 63 / 64 (the
    end of a 64-bin chunk and the start of the next), in the last bin (the partial-chunk walk for bins % 64 != 0), never
    reached, an empty histogram, counts above 2^24.  Many slots with different outcomes in one launch; the torch op on single
    rows agrees."""
    import dipoorlet_amd.torch_ops  # noqa: F401  (registers torch.ops.dipoorlet)
    from dipoorlet_amd import ops
    rng = np.random.default_rng(77)
    for bins in (1, 63, 64, 65, 127, 128, 129, 2048, 2049, 16384):
        cases, thrs = _percentile_cases(bins, rng)
        acc = ops.CalibAccumulators(len(cases), dev, bins)
        acc.set_minmax(torch.tensor([c[1] for c in cases], dtype=torch.float32, device=dev),
                       torch.tensor([c[2] for c in cases], dtype=torch.float32, device=dev))
        acc.hist_prepare()
        acc.hist.copy_(torch.from_numpy(np.stack([c[0] for c in cases])))
        found = set()
        for thr in thrs:
            got = acc.hist_percentile(thr).cpu().numpy()
            for s, (h, gmin, gmax) in enumerate(cases):
                want = np.asarray(O.hist_percentile(h, gmin, gmax, bins, thr), np.float32)
                assert np.array_equal(got[s].view(np.uint32), want.view(np.uint32)), (bins, thr, s, got[s], want)
                found.add(tuple(want.tolist()))
            for s in (0, len(cases) - 1):
                one = torch.ops.dipoorlet.hist_percentile(acc.hist[s].contiguous(), cases[s][1], cases[s][2], thr).cpu().numpy()
                assert np.array_equal(one.view(np.uint32), got[s].view(np.uint32)), (bins, thr, s)
        assert len(found) >= min(bins, 4), bins                 # (the slots do not all give one answer)
    # where fl32(count) decides: counts 2^24 + 1 and 2^24 - 1 over a total of 2^25.  fl32(2^24 + 1) = 2^24, so bin 0 holds exactly
    # 0.5 and a threshold of 0.5 + 2^-25 is reached in bin 1 (with the exact count it would be reached in bin 0)
    h = np.array([(1 << 24) + 1, (1 << 24) - 1], np.int64)
    thr = 0.5 + 2.0 ** -25
    assert (1 << 24) + 1 >= thr * (1 << 25)                     # (exact counts: bin 0)
    want = np.asarray(O.hist_percentile(h, -4.0, 4.0, 2, thr), np.float32)
    assert want[1] == np.float32(1.5 * 4.0 / 2)                 # (the reference's fl32 counts: bin 1)
    got = torch.ops.dipoorlet.hist_percentile(torch.from_numpy(h).to(dev), -4.0, 4.0, thr).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


def test_channel_diff_sum_at_the_shapes_bias_correction_meets(dev):
    """k_channel_diff_sum (bias_correction.py:9-13's sum of fp - q per channel) against fp64 numpy: Gemm outputs [n, C] (the
    lane-per-channel path) with n up to 4096 and C around 64, Conv1d outputs [n, C, L] with L % 4 in {0, 1, 3} from aligned
    bases and from bases one element off, a = 1e6 + δ (the fp64 sum of exact fp32 differences: no cancellation error),
    accumulation over 5 chunks."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(79)
    shapes = [(n, C) for n in (1, 7, 4096) for C in (1, 63, 64, 65, 1000)]
    shapes += [(n, C, L) for n, C in ((3, 5), (8, 64)) for L in (12, 13, 15, 4)]
    for shape in shapes:
        for off in (0, 1):
            size = int(np.prod(shape))
            fa = torch.from_numpy(rng.standard_normal(size + 1).astype(np.float32)).to(dev)
            fb = torch.from_numpy(rng.standard_normal(size + 1).astype(np.float32)).to(dev)
            a, b = fa[off:off + size].reshape(shape), fb[off:off + size].reshape(shape)
            a64, b64 = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
            axes = tuple(i for i in range(len(shape)) if i != 1)
            want = (a64 - b64).sum(axis=axes)
            np.testing.assert_allclose(ops.channel_diff_sum(a, b).cpu().numpy(), want, rtol=1e-12, atol=1e-12,
                                       err_msg=f"{shape} off {off}")
    # cancellation: a = 1e6 + δ, b = 1e6 + δ' (fp32 spacing 1/16 there): every a - b is exact in fp64, so is their sum
    for shape in ((4096, 65), (7, 64), (8, 64, 13), (3, 5, 12)):
        acc, want = None, 0.0
        for _ in range(5):                                       # 5 chunks into one accumulator
            base = np.float32(1e6)
            a = (base + rng.integers(-40, 41, shape).astype(np.float32) / np.float32(16)).astype(np.float32)
            b = (base + rng.integers(-40, 41, shape).astype(np.float32) / np.float32(16)).astype(np.float32)
            acc = ops.channel_diff_sum(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), acc)
            axes = tuple(i for i in range(len(shape)) if i != 1)
            want = want + (a.astype(np.float64) - b.astype(np.float64)).sum(axis=axes)
        np.testing.assert_allclose(acc.cpu().numpy(), want, rtol=1e-12, atol=0, err_msg=str(shape))


def _matmul_f64(a, b):
    """a @ b in fp64 with IEEE semantics for every term (0 * inf = NaN, inf - inf = NaN): BLAS on the finite rows and columns,
    explicit sums of products on the rows of a and the columns of b that hold a NaN or an inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.where(np.isfinite(a), a, 0) @ np.where(np.isfinite(b), b, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in np.nonzero(~np.isfinite(a).all(1))[0]:
            out[m] = (a[m][:, None] * b).sum(0)
        for n in np.nonzero(~np.isfinite(b).all(0))[0]:
            out[:, n] = (a * b[:, n]).sum(1)
    return out


def _same_specials_and_close(got, want, atol):
    """NaN, +inf and -inf exactly where fp64 numpy puts them and nowhere else; the finite values within atol."""
    got = np.asarray(got, np.float64)
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(got), f(want)), (f.__name__, np.argwhere(f(got) != f(want))[:5])
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=atol)


def test_gemm_small_nan_and_inf_stay_in_their_rows_and_columns(dev):
    """dpl_gemm_small with a NaN in one row of A and an inf in one column of B (a whole column and a single element): the result
    holds NaN / ±inf exactly where fp64 numpy does — the NaN row, the inf columns — and nowhere else, at shapes where the padded
    tiles (M % 32, N % 64 != 0) and the split-K sum (K cut into several ranges) would carry them over.  alpha = 0 with a finite
    product gives beta * bias exactly."""
    from dipoorlet_amd import ops
    rng = np.random.default_rng(81)
    for M, K, N, trans_b in [(5, 40, 9, False), (64, 2048, 1000, True), (33, 65, 70, False), (7, 8200, 64, False),
                             (40, 300, 129, True), (1, 1, 1, False)]:
        a = rng.standard_normal((M, K)).astype(np.float32)
        w = rng.standard_normal((K, N)).astype(np.float32)
        a[M - 1, rng.integers(K)] = np.nan                     # a row in the last (partial) row tile
        w[rng.integers(K), N - 1] = np.inf                      # one element: column N-1 is ±inf by the sign of a's entry
        if N > 2:
            w[:, N // 2] = -np.inf                              # a whole column: ±inf terms of both signs, NaN
            w[0, 1] = np.inf                                    # and an inf that meets the NaN row
        bias = rng.standard_normal(N).astype(np.float32)
        bt = torch.from_numpy(w.T.copy()).to(dev).t() if trans_b else torch.from_numpy(w).to(dev)
        for alpha, beta in ((1.0, 1.0), (0.5, -2.0)):
            got = ops.gemm_small(torch.from_numpy(a).to(dev), bt, torch.from_numpy(bias).to(dev), alpha, beta).cpu().numpy()
            with np.errstate(invalid="ignore"):
                want = alpha * _matmul_f64(a, w) + beta * bias.astype(np.float64)
            _same_specials_and_close(got, want, 2e-6 * (np.sqrt(K) * abs(alpha) + abs(beta)) * max(1.0, np.sqrt(K) / 8))
    # alpha = 0, a finite product: beta * bias, bit for bit (0 * a finite sum is a zero)
    for M, K, N in ((33, 65, 70), (7, 8200, 64)):
        a = rng.standard_normal((M, K)).astype(np.float32)
        w = rng.standard_normal((K, N)).astype(np.float32)
        bias = rng.standard_normal((M, N)).astype(np.float32)
        got = ops.gemm_small(torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(bias).to(dev), 0.0, 1.5)
        assert np.array_equal(got.cpu().numpy(), np.float32(1.5) * bias), (M, K, N)


def test_executor_gemm_attributes_and_3d_matmul_vs_onnx_definition(dev):
    """The executor's Gemm against the ONNX definition Y = alpha * A' B' + beta * C in fp64 (A' = A^T when transA = 1, B' = B^T
    when transB = 1; C broadcast from [], [1], [N], [M, 1] or [M, N]), and MatMul with a 3-D left operand."""
    from dipoorlet_amd.executor import _OPS
    from dipoorlet_amd.onnx_io import Node
    rng = np.random.default_rng(85)
    M, K, N = 19, 70, 33
    for trans_a in (0, 1):
        for trans_b in (0, 1):
            for c_shape in ((), (1,), (N,), (M, 1), (M, N)):
                alpha, beta = (0.75, -1.25) if (trans_a + trans_b) % 2 else (2.0, 0.5)
                a = rng.standard_normal((K, M) if trans_a else (M, K)).astype(np.float32)
                b = rng.standard_normal((N, K) if trans_b else (K, N)).astype(np.float32)
                c = rng.standard_normal(c_shape).astype(np.float32)
                node = Node("Gemm", ["a", "b", "c"], ["y"], name="gemm", attrs={"transA": trans_a, "transB": trans_b,
                                                                                 "alpha": alpha, "beta": beta})
                y = _OPS["Gemm"](None, node, *(torch.from_numpy(np.asarray(v)).to(dev) for v in (a, b, c))).cpu().numpy()
                a64, b64 = a.astype(np.float64), b.astype(np.float64)
                want = alpha * ((a64.T if trans_a else a64) @ (b64.T if trans_b else b64)) + beta * c.astype(np.float64)
                assert y.shape == (M, N), (trans_a, trans_b, c_shape)
                np.testing.assert_allclose(y, want, rtol=0, atol=2e-6 * (np.sqrt(K) * abs(alpha) + abs(beta)) * 4,
                                           err_msg=f"transA={trans_a} transB={trans_b} C{c_shape}")
    a = rng.standard_normal((2, 17, 96)).astype(np.float32)
    b = rng.standard_normal((96, 40)).astype(np.float32)
    y = _OPS["MatMul"](None, None, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
    assert y.shape == (2, 17, 40)
    np.testing.assert_allclose(y, a.astype(np.float64) @ b.astype(np.float64), rtol=0, atol=2e-6 * np.sqrt(96) * 4)
