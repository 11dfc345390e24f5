"""CPU ORACLE (test infrastructure, NOT product code) — restatement of the reference's AdaRound / BRECQ / QDrop
arithmetic with every gradient written out by hand.

  * Only tests/ may import this module; the product package never does.
  * The reference expresses these as torch expressions and lets autograd differentiate them
    (dipoorlet/weight_transform/ada_quant_layer.py:28-125, adaround.py:119-144, torch.optim.Adam).  Here the
    forward values AND the derivatives autograd would produce are explicit numpy fp32 formulas — including the
    corners that matter for parity: clamp() passes its gradient on the closed interval, maximum / minimum split
    it on ties, pow(x, 0.0) has zero gradient, round() has none — so that the HIP kernels can be checked against
    something that is not the same autograd graph.
  * Parity pin: tests/test_round_oracle_golden.py checks every function against tests/golden/round_level.*,
    produced by tests/golden/gen_golden_round.py from the reference's own code on CPU torch.
    The same file pins Sgd to torch.optim.SGD bit for bit and the rows with one NaN / ±inf (tests/round_cases.py)
    to CPU torch autograd evaluating the reference's expressions.
  * Matrix products / convolutions inside `train_layer` use torch's CPU kernels (third-party numerics; the
    reference uses the same library on the GPU).
"""
import math

import numpy as np

F32 = np.float32
ZETA, GAMMA = 1.1, -0.1
ZG = F32(ZETA - GAMMA)      # torch casts the python scalar to the tensor dtype
G32 = F32(GAMMA)


def sigmoid(a):
    a = np.asarray(a, F32)
    with np.errstate(over="ignore"):             # exp(-a) = inf for a < -88.7: the sigmoid is 0 there
        return (F32(1) / (F32(1) + np.exp(-a, dtype=F32))).astype(F32)


def rect_sigmoid(mask, inside=None):
    """ada_quant_layer.py:105-106 -> (h, dh/dmask).  clamp(0, 1) passes the gradient where 0 <= raw <= 1.
    `inside` (tests of the kink, where one ulp of exp decides): a boolean array that replaces that decision."""
    sg = sigmoid(mask)
    raw = (ZG * sg + G32).astype(F32)
    h = np.clip(raw, F32(0), F32(1)).astype(F32)
    inside = ((raw >= 0) & (raw <= 1)) if inside is None else inside
    dh = np.where(inside, (ZG * (F32(1) - sg)).astype(F32) * sg, F32(0)).astype(F32)
    # a NaN mask: clamp's backward hands on a zero, sigmoid's multiplies it by NaN -> NaN (h is NaN through np.clip)
    return h, np.where(np.isnan(raw), raw, dh).astype(F32)


def _bc(v, ndim):
    v = np.asarray(v, F32).reshape(-1)
    return v.reshape([-1] + [1] * (ndim - 1)) if v.size > 1 else v.reshape([1] * ndim)


def alpha_init(w, scale):
    """adaround.py:67 + ada_quant_layer.py:147: rest = w/s - floor(w/s); mask = -log((zeta-gamma)/(rest-gamma) - 1).
    torch evaluates `scalar / tensor` as reciprocal(tensor) * scalar."""
    w = np.asarray(w, F32)
    t = (w / _bc(scale, w.ndim)).astype(F32)
    wf = np.floor(t).astype(F32)
    with np.errstate(invalid="ignore"):          # w = ±inf: inf - inf, the mask is NaN as in torch
        rest = (t - wf).astype(F32)
        inv = (F32(1) / (rest - G32).astype(F32)).astype(F32)
        return wf, (-np.log((inv * ZG).astype(F32) - F32(1), dtype=F32)).astype(F32)


def _clamp_with_pass(v, q_min, q_max):
    """torch.max(v, q_min) then torch.min(., q_max) and the factor autograd applies to the incoming gradient:
    where(a == b, grad / 2, grad).masked_fill(a < b, 0) — a NaN compares false both times, so it takes the WHOLE
    gradient (and np.maximum / np.minimum hand the NaN on, as torch.max / torch.min do)."""
    f_lo = np.where(v == q_min, F32(0.5), np.where(v < q_min, F32(0), F32(1)))
    v1 = np.maximum(v, q_min)
    f_hi = np.where(v1 == q_max, F32(0.5), np.where(v1 > q_max, F32(0), F32(1)))
    return np.minimum(v1, q_max).astype(F32), (f_lo * f_hi).astype(F32)


def quant_weight(w, mask, scale, q_min, q_max, per_channel, soft=True, inside=None):
    """ada_quant_layer.py:39-50 -> (quantised weight, d(quantised weight)/d(mask)).  Only the per-channel branch
    clamps (the per-tensor branch calls weight.clamp(...) without using the result)."""
    w = np.asarray(w, F32)
    s = _bc(scale, w.ndim)
    wf = np.floor((w / s).astype(F32)).astype(F32)
    if soft:
        h, dh = rect_sigmoid(mask, inside)
    else:
        h, dh = (np.asarray(mask, F32) >= 0).astype(F32), np.zeros_like(w)
    v = (wf + h).astype(F32)
    passf = np.ones_like(w)
    if per_channel:
        v, passf = _clamp_with_pass(v, _bc(q_min, w.ndim), _bc(q_max, w.ndim))
    return (v * s).astype(F32), (np.broadcast_to(s, w.shape) * passf * dh).astype(F32)


def temp_decay(t, t_max, rel_start_decay=0.2, start_b=20, end_b=2):
    """ada_quant_layer.py:119-134."""
    start = rel_start_decay * t_max
    if t < start:
        return 0.0
    rel_t = (t - start) / (t_max - start)
    return end_b + 0.5 * (start_b - end_b) * (1 + np.cos(rel_t * np.pi))


def reg_value_grad(mask, beta, lam=0.01, inside=None):
    """ada_quant_layer.py:108-110: lam * sum(1 - (|h - 0.5| * 2)^beta) and its gradient w.r.t. the mask.
    beta == 0: pow(x, 0) = 1 everywhere and torch defines its gradient as zero."""
    h, dh = rect_sigmoid(mask, inside)
    if beta == 0.0:
        return 0.0, np.zeros_like(h)
    b = F32(beta)
    d = (h - F32(0.5)).astype(F32)
    u = (np.abs(d) * F32(2)).astype(F32)
    val = lam * float(np.sum((F32(1) - np.power(u, b, dtype=F32)).astype(np.float64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        dp = np.where(u > 0, b * np.power(u, b - F32(1), dtype=F32), F32(0)).astype(F32)
    g = (F32(-lam) * dp * F32(2) * np.sign(d).astype(F32) * dh).astype(F32)
    return val, g


def l2_value_grad(pred, tgt, relu=False):
    """ada_quant_layer.py:115-116: ((pred - tgt)^2).sum(1).mean() and d/d(pred); with relu the loss is taken on
    max(pred, 0) and the ReLU's gradient (pred > 0) is folded in."""
    pred, tgt = np.asarray(pred, F32), np.asarray(tgt, F32)
    m = pred.size // pred.shape[1]
    y = np.maximum(pred, F32(0)) if relu else pred
    d = (y - tgt).astype(F32)
    val = float(np.sum((d * d).astype(np.float64))) / m
    g = (F32(F32(1.0 / m) * F32(2)) * d).astype(F32)
    if relu:                                      # threshold_backward: 0 where pred <= 0 — a NaN pred keeps its NaN
        g = np.where(pred <= 0, F32(0), g).astype(F32)
    return val, g


def quant_acti_drop(x, r, scale, q_min, q_max, prob):
    """ada_quant_layer.py:28-36 with the uniform draw `r` given -> (y, dy/dx as a 0/1 mask): round() blocks the
    gradient, the kept (un-quantised) elements pass it."""
    x = np.asarray(x, F32)
    q = np.rint((x / F32(scale)).astype(F32)).astype(F32)      # torch.round: half to even
    q = (np.minimum(np.maximum(q, F32(q_min)), F32(q_max)) * F32(scale)).astype(F32)
    if r is None or prob >= 1.0:
        return q, np.zeros_like(x)
    keep_q = np.asarray(r, F32) < F32(prob)
    return np.where(keep_q, q, x).astype(F32), np.where(keep_q, F32(0), F32(1)).astype(F32)


def sparse_quant(w, mask, scale, q_min, q_max, per_channel):
    """sparse_quant_layer.py:9-29 on the pruned weight w * mask (mask None: w itself) -> (quantised weight, the factor
    the clamp applies to the straight-through gradient).  round() is half to even; only the per-channel branch clamps
    (the per-tensor branch discards its clamp), with the tie split of torch.max / torch.min."""
    w = np.asarray(w, F32)
    s = _bc(scale, w.ndim)
    wm = w if mask is None else (w * np.asarray(mask, F32)).astype(F32)
    v = np.rint((wm / s).astype(F32)).astype(F32)
    passf = np.ones_like(w)
    if per_channel:
        v, passf = _clamp_with_pass(v, _bc(q_min, w.ndim), _bc(q_max, w.ndim))
    return (v * s).astype(F32), np.broadcast_to(passf, w.shape).astype(F32)


def sparse_grad(G, mask, scale, passf, grad_scale=1.0):
    """dL/dw for upstream dL/d(qw) = G (times grad_scale: DDP's mean) back through `* scale`, the clamp, the
    straight-through round, `/ scale` and `* mask`, in autograd's order."""
    G = np.asarray(G, F32)
    s = _bc(scale, G.ndim)
    g = ((((G * F32(grad_scale)).astype(F32) * s).astype(F32) * passf).astype(F32) / s).astype(F32)
    return g if mask is None else (g * np.asarray(mask, F32)).astype(F32)


def fma32(a, b, c):
    """fp32 fused multiply-add a * b + c with ONE rounding.  The product of two fp32 is exact in fp64; the fp64 sum is
    rounded to odd (TwoSum gives the sum's exact error), after which the cast to fp32 rounds as the exact value would."""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, F32).astype(np.float64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


class Sgd:
    """torch.optim.SGD (momentum, weight decay; dampening 0, no Nesterov), single-tensor form:
    g = g.add(w, alpha=wd) [skipped for wd == 0]; buf = g on the first step, else buf.mul_(momentum).add_(g);
    w.add_(buf, alpha=-lr).  torch's add(other, alpha=) is ONE fused multiply-add per element (vec::fmadd in its CPU
    kernels, `a + alpha * b` under the device compilers' default contraction); mul_ then add_ are two roundings."""

    def __init__(self, lr=1e-3, momentum=0.9, weight_decay=1e-4):
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.buf = None

    def step(self, w, g, lr=None):
        """-> the updated weight; self.buf is the momentum buffer after the step."""
        w, g = np.asarray(w, F32), np.asarray(g, F32)
        if self.weight_decay != 0:
            g = fma32(F32(self.weight_decay), w, g)
        if self.buf is None:
            self.buf = g.copy()
        else:
            self.buf = ((self.buf * F32(self.momentum)).astype(F32) + g).astype(F32)
        return fma32(F32(-(self.lr if lr is None else lr)), self.buf, w)


def sched_fields(t, adam_step, t_max, lr=1e-3, b1=0.9, b2=0.999):
    """What dpl_round_sched_advance writes for iteration t (0-based) entering Adam step `adam_step` (1-based):
    (reg_beta, step_size, bc2_sqrt), computed in python doubles as TempDecay and torch.optim.Adam do, then cast."""
    return (F32(temp_decay(t, t_max)), F32(lr / (1.0 - b1 ** adam_step)), F32(math.sqrt(1.0 - b2 ** adam_step)))


class Adam:
    """torch.optim.Adam, single-tensor form (lr 1e-3, betas (0.9, 0.999), eps 1e-8): lerp, addcmul, addcdiv with the
    python-double scalars cast to fp32 at the op."""

    def __init__(self, shape, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
        self.m, self.v, self.t = np.zeros(shape, F32), np.zeros(shape, F32), 0
        self.lr, self.b1, self.b2, self.eps = lr, b1, b2, eps

    def step(self, p, g):
        self.t += 1
        g = np.asarray(g, F32)
        self.m = (self.m + F32(1 - self.b1) * (g - self.m).astype(F32)).astype(F32)
        self.v = ((self.v * F32(self.b2)).astype(F32) + (F32(1 - self.b2) * g).astype(F32) * g).astype(F32)
        step_size = self.lr / (1 - self.b1 ** self.t)
        bc2_sqrt = math.sqrt(1 - self.b2 ** self.t)
        denom = ((np.sqrt(self.v) / F32(bc2_sqrt)).astype(F32) + F32(self.eps)).astype(F32)
        return (p + ((F32(-step_size) * self.m).astype(F32) / denom).astype(F32)).astype(F32)


def train_layer(kind, w, b, x, fp, scale, q_min, q_max, per_channel, relu, bs, epochs, snapshots=()):
    """learning_round_mask (adaround.py:119-144) for ONE Gemm ('gemm': y = x W^T + b) or 3x3 / pad-1 Conv ('conv')
    layer, no DDP: returns (final mask, {step: mask}, hard-rounded weight)."""
    import torch
    import torch.nn.functional as F
    n = x.shape[0]
    nb = int(math.ceil(n / bs))
    total = epochs * nb
    _, mask = alpha_init(w, scale)
    opt = Adam(mask.shape)
    xt, bt = torch.from_numpy(np.asarray(x, F32)), torch.from_numpy(np.asarray(b, F32))
    snaps, cur = {}, 0
    for _ in range(epochs):
        for i in range(nb):
            qw, dqw = quant_weight(w, mask, scale, q_min, q_max, per_channel)
            qwt = torch.from_numpy(qw).requires_grad_(True)
            xb = xt[i * bs:(i + 1) * bs]
            z = F.linear(xb, qwt, bt) if kind == "gemm" else F.conv2d(xb, qwt, bt, 1, 1)
            _, gz = l2_value_grad(z.detach().numpy(), fp[i * bs:(i + 1) * bs], relu)
            z.backward(torch.from_numpy(gz))
            _, greg = reg_value_grad(mask, temp_decay(cur, total))
            g = (qwt.grad.numpy() * dqw).astype(F32) + greg
            mask = opt.step(mask, g)
            cur += 1
            if cur in snapshots:
                snaps[cur] = mask.copy()
    hard, _ = quant_weight(w, mask, scale, q_min, q_max, per_channel, soft=False)
    return mask, snaps, hard
