"""`torch.ops.dipoorlet.*` — the custom-op spelling of the kernel library, for callers that live in
torch (ORT-IOBinding / eager pipelines, torch.compile graphs).  Registrations over dipoorlet_amd.ops: every op runs
the HIP kernels on the current stream and is registered for the 'cuda' (ROCm) device only — there is no CPU
implementation to fall back to.

Per tensor:
    dipoorlet::minmax(Tensor x) -> Tensor                      [2] fp32 (min, max); NaN if x holds one
    dipoorlet::abs_hist_(Tensor x, float dmax, int bins, Tensor(a!) hist) -> ()      hist += np.histogram(|x|, bins, (0, dmax))
    dipoorlet::hist_percentile(Tensor hist, float gmin, float gmax, float threshold) -> Tensor   [2] fp32 clip
    dipoorlet::hist_kl(Tensor hist, float gmin, float gmax, int levels) -> Tensor                [2] fp32 clip (entropy search)
    dipoorlet::hist_qmse(Tensor hist, float gmin, float gmax, str qtype, int bit_width, int first) -> Tensor   [2] fp32 clip (quantisation-MSE search)
    dipoorlet::octav(Tensor x, bool dynamic_sym) -> Tensor     [3] fp32 (s, min, max) (forward_net.py:315-330)
    dipoorlet::rowwise_minmax(Tensor w2d) -> (Tensor, Tensor)
    dipoorlet::colwise_absmax(Tensor x) -> Tensor              [C] fp32: max |x| per channel of a channels-last x (ops.colwise_absmax)
    dipoorlet::fake_quant(Tensor x, Tensor scale, Tensor zero_point, int axis, int qlo, int qhi) -> Tensor
    dipoorlet::fake_quant_relu(Tensor x, Tensor scale, Tensor zero_point, int axis, int qlo, int qhi) -> Tensor          fq(relu(x))
    dipoorlet::fake_quant_add_relu(Tensor x, Tensor x2, Tensor scale, Tensor zero_point, int axis, int qlo, int qhi) -> Tensor
    dipoorlet::fake_quant_fp8(Tensor x, Tensor scale, int axis) -> Tensor      the pair on the OCP FP8 E4M3 grid (ops.fake_quant_fp8)
    dipoorlet::fake_quant_mx(Tensor x, int axis, str elem) -> Tensor           the OCP Microscaling pair, 'mxfp8' / 'mxfp6_e2m3' / 'mxfp6_e3m2' / 'mxfp4', blocks of 32 along axis (ops.fake_quant_mx)
    dipoorlet::mx_encode(Tensor x, int axis, str elem) -> (Tensor, Tensor)     the same values as bytes: (element codes, E8M0 scales), uint8, K-innermost (ops.mx_encode: --mx_pack)
    dipoorlet::mx_decode(Tensor codes, Tensor scales, str elem, int[] shape, int axis) -> Tensor   those bytes back to fp32 of `shape` (ops.mx_decode)
    dipoorlet::mx_gemm(Tensor a_codes, Tensor a_scales, Tensor b_codes, Tensor b_scales, str elem_a, str elem_b) -> Tensor
                                                               two packed operands through the block-scaled matrix instruction, fp32 [*batch, m, n] (ops.mx_gemm: --mx_verify)
    dipoorlet::mx_scale_search(Tensor x, int axis, str elem) -> Tensor         uint8, one E8M0 byte per block: the floor rule's or one more, whichever errs less (ops.mx_scale_search: --mx_scale_search)
    dipoorlet::fake_quant_mx_scaled(Tensor x, int axis, str elem, Tensor scales) -> Tensor   the MX pair under those given bytes (ops.fake_quant_mx_scaled)
    dipoorlet::hadamard32(Tensor x) -> Tensor                           x . blockdiag(H32) along the last axis, a multiple of 32 (ops.hadamard32: --mx_rotate)
    dipoorlet::gptq_block(Tensor(a!) w, int c0, int nb, Tensor u, Tensor scale, Tensor zero_point, int qlo, int qhi, str fmt) -> Tensor
                                                               one block of GPTQ's column recursion in place on w; -> Err [rows, nb] (ops.gptq_block)
    dipoorlet::gptq_mx_block(Tensor(a!) w, int c0, int nb, Tensor u, str elem) -> (Tensor, Tensor)
                                                               the same on an MX block-scaled grid; -> (Err [rows, nb], E8M0 entry bytes uint8 [rows, ceil(K / 32)]) (ops.gptq_mx_block: --mx_gptq)
Over every tensor of a batch of images in ONE launch — what the reference's loops over `ort_outputs` stand for
(forward_net.py:220-235, 265-280, 314-340); xs[t] is tensor t of the batch, [B, ...] contiguous fp32:
    dipoorlet::minmax_batched(Tensor[] xs, Tensor(a!) mins, Tensor(b!) maxs) -> ()   running min / max per tensor, [T] fp32
    dipoorlet::abs_hist_batched_(Tensor[] xs, Tensor mins, Tensor maxs, int bins, Tensor(a!) hist) -> ()
                                                               hist[t] += np.histogram(|xs[t]|, bins, (0, max(|mins[t]|, |maxs[t]|)))
    dipoorlet::octav_batched(Tensor[] xs, bool dynamic_sym) -> Tensor                 [B, T, 3] fp32 (s, min, max) per (image, tensor)
    dipoorlet::fake_quant_set(Tensor[] xs, Tensor[] scales, Tensor[] zero_points, int[] inner, int[] qlo, int[] qhi) -> Tensor[]

No allocation inside except the outputs (hist_kl / hist_qmse: and the two workspace outputs of the C ABI, `best` and `div` / `err`,
three allocations in all), no host synchronisation: everything a launch needs besides its inputs — the work
decomposition of the tensor set, the pointer-table slots, accumulators, OCTAV workspace — belongs to a plan cached on
(per-image sizes, batch, device) and is built by the FIRST call with that key; later calls only launch.  The OCTAV ops run the
exact-tail form on the caller's stream (ops.octav_batch(inline=True)): the rare pairs that neither the walk nor the rescue finish
(values of 2^14 and above or +-inf, a log bin of 2^20 values or more) take the compaction route in the same stream order, on a
whole-batch fallback block the plan allocates with its first OCTAV call — 8 bytes per element of the batch, twice the batch's
activations, held as long as the plan is cached.  Nothing is read back: the rows are final once the caller's stream reaches them,
and no reference to the inputs outlives the call.  (A set with a pair above 64 slices runs the two-read form, as octav_batch does.)
"""
import ctypes
from typing import List, Tuple

import torch

from . import _hip, ops

_PLANS = {}
_PLANS_MAX = 32
_RANGE = {}          # device index -> fp32 [2]: the (gmin, gmax) argument of hist_percentile / hist_kl


class _Cached:
    """Everything the ops need for one (per-image sizes, batch, device) besides inputs and outputs."""

    def __init__(self, elems, batch, device):
        self.plan = ops.TensorSetPlan(elems, batch, device)
        self.device = device
        self.acc = {}        # bins -> CalibAccumulators (min / max encodings, histogram ranges; hist: the caller's tensor)
        self.octav_done = torch.cuda.Event()    # behind the last OCTAV call: its workspace is the plan's one set of buffers
        self.fq = {}         # parameter identity -> FakeQuantSet

    def accumulators(self, bins):
        a = self.acc.get(bins)
        if a is None:
            a = self.acc[bins] = ops.CalibAccumulators(self.plan.T, self.device, bins)
            a.ranges = torch.empty(a.n * ctypes.sizeof(_hip.HistRange), dtype=torch.uint8, device=self.device)
        return a


def _cached(xs, batch=None):
    """The cached plan for this tensor set: xs[t] = tensor t of a batch of `batch` images (default: xs[0].shape[0])."""
    if not xs:
        raise ValueError("an empty tensor list")
    b = int(batch if batch is not None else (xs[0].shape[0] if xs[0].dim() > 0 else 1))
    if b < 1 or any(x.numel() % b for x in xs):     # (a per-tensor op passes batch = 1)
        raise ValueError(f"every tensor must hold a whole number of elements per image (batch {b})")
    dev = xs[0].device
    key = (tuple(x.numel() // b for x in xs), b, dev.index)
    c = _PLANS.get(key)
    if c is None:
        if len(_PLANS) >= _PLANS_MAX:
            _PLANS.pop(next(iter(_PLANS)))
        c = _PLANS[key] = _Cached(list(key[0]), b, dev)
    return c


def _contig(xs):
    return [x if x.is_contiguous() else x.contiguous() for x in xs]


# ---------------------------------------------------------------------------------------------- min / max
@torch.library.custom_op("dipoorlet::minmax", mutates_args=(), device_types="cuda")
def minmax(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    c = _cached([x], 1)
    a = c.accumulators(2048)
    a.reset_minmax()
    a.minmax_accumulate(c.plan, [x])
    lo, hi = a.finalize_minmax()
    return torch.cat([lo, hi])


@minmax.register_fake
def _(x):
    return x.new_empty(2, dtype=torch.float32)


@torch.library.custom_op("dipoorlet::minmax_batched", mutates_args=("mins", "maxs"), device_types="cuda")
def minmax_batched(xs: List[torch.Tensor], mins: torch.Tensor, maxs: torch.Tensor) -> None:
    xs = _contig(xs)
    c = _cached(xs, 1)          # (one slot per tensor: the images of a batch merge for free)
    if mins.numel() != c.plan.T or maxs.numel() != c.plan.T or mins.dtype != torch.float32 or maxs.dtype != torch.float32:
        raise ValueError("mins / maxs must be fp32 tensors with one entry per tensor of xs")
    a = c.accumulators(2048)
    a.reset_minmax()
    a.minmax_accumulate(c.plan, xs)
    lo, hi = a.finalize_minmax()
    # running form: NaN (from either side) propagates like numpy's min / max (torch.minimum / maximum propagate NaN)
    torch.minimum(mins, lo.view(mins.shape), out=mins)
    torch.maximum(maxs, hi.view(maxs.shape), out=maxs)


# ---------------------------------------------------------------------------------------------- histograms
def _hist_into(c, xs, bins, hist):
    a = c.accumulators(bins)
    L = _hip.lib()
    _hip.check(L.dpl_hist_prepare(ops._ptr(a.gmin), ops._ptr(a.gmax), a.n, a.bins, ops._ptr(a.ranges), ops._stream()), "dpl_hist_prepare")
    tab = c.plan.seg_table(xs)
    w = c.plan.work("hist")
    _hip.check(L.dpl_abs_hist_accumulate(*w.args(), ops._ptr(tab), ops._ptr(a.ranges), a.bins, ops._ptr(hist), ops._stream()),
               "dpl_abs_hist_accumulate")


@torch.library.custom_op("dipoorlet::abs_hist_", mutates_args=("hist",), device_types="cuda")
def abs_hist_(x: torch.Tensor, dmax: float, bins: int, hist: torch.Tensor) -> None:
    if hist.dtype != torch.int64 or hist.numel() != bins or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous int64 tensor with `bins` entries")
    x = x.contiguous()
    c = _cached([x], 1)
    a = c.accumulators(int(bins))
    a.gmin.fill_(0.0)
    a.gmax.fill_(float(dmax))
    _hist_into(c, [x], int(bins), hist)


@torch.library.custom_op("dipoorlet::abs_hist_batched_", mutates_args=("hist",), device_types="cuda")
def abs_hist_batched_(xs: List[torch.Tensor], mins: torch.Tensor, maxs: torch.Tensor, bins: int, hist: torch.Tensor) -> None:
    xs = _contig(xs)
    c = _cached(xs, 1)
    T = c.plan.T
    if hist.dtype != torch.int64 or hist.numel() != T * bins or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous int64 tensor [T, bins]")
    if mins.numel() != T or maxs.numel() != T:
        raise ValueError("mins / maxs must hold one entry per tensor of xs")
    a = c.accumulators(int(bins))
    a.gmin.copy_(mins.view(-1))
    a.gmax.copy_(maxs.view(-1))
    _hist_into(c, xs, int(bins), hist)


def _range_of(hist, gmin, gmax):
    """The device's fp32 [2] holding (gmin, gmax), filled on the current stream."""
    rng = _RANGE.get(hist.device.index)
    if rng is None:
        rng = _RANGE[hist.device.index] = torch.empty(2, dtype=torch.float32, device=hist.device)
    rng[0].fill_(float(gmin))
    rng[1].fill_(float(gmax))
    return rng


@torch.library.custom_op("dipoorlet::hist_percentile", mutates_args=(), device_types="cuda")
def hist_percentile(hist: torch.Tensor, gmin: float, gmax: float, threshold: float) -> torch.Tensor:
    if hist.dtype != torch.int64 or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous int64 tensor")
    bins = hist.numel()
    rng = _range_of(hist, gmin, gmax)
    clip = torch.empty(2, dtype=torch.float32, device=hist.device)
    _hip.check(_hip.lib().dpl_hist_percentile(ops._ptr(hist), ops._ptr(rng[0:1]), ops._ptr(rng[1:2]), 1, bins, float(threshold),
                                              ops._ptr(clip), ops._stream()), "dpl_hist_percentile")
    return clip


@hist_percentile.register_fake
def _(hist, gmin, gmax, threshold):
    return hist.new_empty(2, dtype=torch.float32)


@torch.library.custom_op("dipoorlet::hist_kl", mutates_args=(), device_types="cuda")
def hist_kl(hist: torch.Tensor, gmin: float, gmax: float, levels: int) -> torch.Tensor:
    if hist.dtype != torch.int64 or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous int64 tensor")
    bins = hist.numel()
    rng = _range_of(hist, gmin, gmax)
    clip = torch.empty(2, dtype=torch.float32, device=hist.device)
    best = torch.empty(1, dtype=torch.int32, device=hist.device)
    div = torch.empty(bins + 1, dtype=torch.float64, device=hist.device)      # (the search's workspace: an output of the C ABI)
    _hip.check(_hip.lib().dpl_hist_kl(ops._ptr(hist), ops._ptr(rng[0:1]), ops._ptr(rng[1:2]), 1, bins, int(levels), ops._ptr(div),
                                      ops._ptr(best), ops._ptr(clip), ops._stream()), "dpl_hist_kl")
    return clip


@hist_kl.register_fake
def _(hist, gmin, gmax, levels):
    return hist.new_empty(2, dtype=torch.float32)


@torch.library.custom_op("dipoorlet::hist_qmse", mutates_args=(), device_types="cuda")
def hist_qmse(hist: torch.Tensor, gmin: float, gmax: float, qtype: str, bit_width: int, first: int) -> torch.Tensor:
    if hist.dtype != torch.int64 or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous int64 tensor")
    bins = hist.numel()
    grid, top = ops.qmse_grid(qtype, bit_width)
    rng = _range_of(hist, gmin, gmax)
    clip = torch.empty(2, dtype=torch.float32, device=hist.device)
    best = torch.empty(1, dtype=torch.int32, device=hist.device)
    err = torch.empty(bins + 1, dtype=torch.float64, device=hist.device)      # (the search's workspace: an output of the C ABI)
    _hip.check(_hip.lib().dpl_hist_qmse(ops._ptr(hist), ops._ptr(rng[0:1]), ops._ptr(rng[1:2]), 1, bins, int(first), grid, top,
                                        ops._ptr(err), ops._ptr(best), ops._ptr(clip), ops._stream()), "dpl_hist_qmse")
    return clip


@hist_qmse.register_fake
def _(hist, gmin, gmax, qtype, bit_width, first):
    return hist.new_empty(2, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- OCTAV
def _octav(xs, dynamic_sym, batch=None):
    xs = _contig(xs)
    c = _cached(xs, batch)
    stream = torch.cuda.current_stream(c.device)
    stream.wait_event(c.octav_done)     # (a caller that switches streams: the last call's kernels are done with the workspace)
    out = ops.octav_batch(c.plan, xs, dynamic_sym, inline=True)
    c.octav_done.record(stream)
    return out


@torch.library.custom_op("dipoorlet::octav", mutates_args=(), device_types="cuda")
def octav(x: torch.Tensor, dynamic_sym: bool) -> torch.Tensor:
    return _octav([x], dynamic_sym, 1).reshape(3)


@octav.register_fake
def _(x, dynamic_sym):
    return x.new_empty(3, dtype=torch.float32)


@torch.library.custom_op("dipoorlet::octav_batched", mutates_args=(), device_types="cuda")
def octav_batched(xs: List[torch.Tensor], dynamic_sym: bool) -> torch.Tensor:
    return _octav(xs, dynamic_sym)


@octav_batched.register_fake
def _(xs, dynamic_sym):
    return xs[0].new_empty(xs[0].shape[0], len(xs), 3, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- weights, fake quant
@torch.library.custom_op("dipoorlet::rowwise_minmax", mutates_args=(), device_types="cuda")
def rowwise_minmax(w2d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.rowwise_minmax(w2d.contiguous())


@rowwise_minmax.register_fake
def _(w2d):
    return w2d.new_empty(w2d.shape[0]), w2d.new_empty(w2d.shape[0])


@torch.library.custom_op("dipoorlet::colwise_absmax", mutates_args=(), device_types="cuda")
def colwise_absmax(x: torch.Tensor) -> torch.Tensor:
    return ops.colwise_absmax(x.contiguous())


@colwise_absmax.register_fake
def _(x):
    return x.new_empty(x.shape[-1], dtype=torch.float32)


@torch.library.custom_op("dipoorlet::fake_quant", mutates_args=(), device_types="cuda")
def fake_quant(x: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor, axis: int, qlo: int,
               qhi: int) -> torch.Tensor:
    return ops.fake_quant(x.contiguous(), scale, zero_point, qlo, qhi, axis=axis if scale.numel() > 1 else None)


@fake_quant.register_fake
def _(x, scale, zero_point, axis, qlo, qhi):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("dipoorlet::fake_quant_relu", mutates_args=(), device_types="cuda")
def fake_quant_relu(x: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor, axis: int, qlo: int,
                    qhi: int) -> torch.Tensor:
    return ops.fake_quant(x.contiguous(), scale, zero_point, qlo, qhi, axis=axis if scale.numel() > 1 else None, pre="relu")


@fake_quant_relu.register_fake
def _(x, scale, zero_point, axis, qlo, qhi):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("dipoorlet::fake_quant_add_relu", mutates_args=(), device_types="cuda")
def fake_quant_add_relu(x: torch.Tensor, x2: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor, axis: int, qlo: int,
                        qhi: int) -> torch.Tensor:
    return ops.fake_quant(x.contiguous(), scale, zero_point, qlo, qhi, axis=axis if scale.numel() > 1 else None, pre="add_relu",
                          x2=x2.contiguous())


@fake_quant_add_relu.register_fake
def _(x, x2, scale, zero_point, axis, qlo, qhi):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("dipoorlet::fake_quant_fp8", mutates_args=(), device_types="cuda")
def fake_quant_fp8(x: torch.Tensor, scale: torch.Tensor, axis: int) -> torch.Tensor:
    return ops.fake_quant_fp8(x.contiguous(), scale, axis=axis if scale.numel() > 1 else None)


@fake_quant_fp8.register_fake
def _(x, scale, axis):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("dipoorlet::fake_quant_mx", mutates_args=(), device_types="cuda")
def fake_quant_mx(x: torch.Tensor, axis: int, elem: str) -> torch.Tensor:
    return ops.fake_quant_mx(x.contiguous(), axis, elem)


@fake_quant_mx.register_fake
def _(x, axis, elem):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("dipoorlet::mx_encode", mutates_args=(), device_types="cuda")
def mx_encode(x: torch.Tensor, axis: int, elem: str) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.mx_encode(x.contiguous(), axis, elem)


@mx_encode.register_fake
def _(x, axis, elem):
    cs, ss = ops.mx_packed_shapes(x.shape, axis, elem)
    return x.new_empty(cs, dtype=torch.uint8), x.new_empty(ss, dtype=torch.uint8)


@torch.library.custom_op("dipoorlet::mx_decode", mutates_args=(), device_types="cuda")
def mx_decode(codes: torch.Tensor, scales: torch.Tensor, elem: str, shape: List[int], axis: int) -> torch.Tensor:
    return ops.mx_decode(codes.contiguous(), scales.contiguous(), elem, shape, axis)


@mx_decode.register_fake
def _(codes, scales, elem, shape, axis):
    return codes.new_empty(list(shape), dtype=torch.float32)


@torch.library.custom_op("dipoorlet::mx_gemm", mutates_args=(), device_types="cuda")
def mx_gemm(a_codes: torch.Tensor, a_scales: torch.Tensor, b_codes: torch.Tensor, b_scales: torch.Tensor, elem_a: str, elem_b: str) -> torch.Tensor:
    return ops.mx_gemm(a_codes.contiguous(), a_scales.contiguous(), b_codes.contiguous(), b_scales.contiguous(), elem_a, elem_b)


@mx_gemm.register_fake
def _(a_codes, a_scales, b_codes, b_scales, elem_a, elem_b):
    return a_codes.new_empty(list(a_codes.shape[:-1]) + [b_codes.shape[-2]], dtype=torch.float32)


@torch.library.custom_op("dipoorlet::mx_scale_search", mutates_args=(), device_types="cuda")
def mx_scale_search(x: torch.Tensor, axis: int, elem: str) -> torch.Tensor:
    return ops.mx_scale_search(x.contiguous(), axis, elem)


@mx_scale_search.register_fake
def _(x, axis, elem):
    return x.new_empty(ops._mx_block_shape(x.shape, axis % x.dim()), dtype=torch.uint8)


@torch.library.custom_op("dipoorlet::fake_quant_mx_scaled", mutates_args=(), device_types="cuda")
def fake_quant_mx_scaled(x: torch.Tensor, axis: int, elem: str, scales: torch.Tensor) -> torch.Tensor:
    return ops.fake_quant_mx_scaled(x.contiguous(), axis, elem, scales.contiguous())


@fake_quant_mx_scaled.register_fake
def _(x, axis, elem, scales):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("dipoorlet::hadamard32", mutates_args=(), device_types="cuda")
def hadamard32(x: torch.Tensor) -> torch.Tensor:
    return ops.hadamard32(x.contiguous())


@hadamard32.register_fake
def _(x):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("dipoorlet::gptq_block", mutates_args=("w",), device_types="cuda")
def gptq_block(w: torch.Tensor, c0: int, nb: int, u: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor, qlo: int, qhi: int,
               fmt: str) -> torch.Tensor:
    """fmt 'int' or 'e4m3' (zero_point, qlo, qhi are not read for 'e4m3'); w, u: contiguous fp32 matrices."""
    return ops.gptq_block(w, c0, nb, u, ops.GptqGrid(fmt, scale, zero_point, qlo, qhi))


@gptq_block.register_fake
def _(w, c0, nb, u, scale, zero_point, qlo, qhi, fmt):
    return w.new_empty((w.shape[0], nb), dtype=torch.float32)


@torch.library.custom_op("dipoorlet::gptq_mx_block", mutates_args=("w",), device_types="cuda")
def gptq_mx_block(w: torch.Tensor, c0: int, nb: int, u: torch.Tensor, elem: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """elem 'mxfp8' or 'mxfp4' (the two mxfp6 formats are refused: the recursion is held to two grids); w, u: contiguous fp32 matrices; whole MX blocks only (ops.gptq_mx_block)."""
    return ops.gptq_mx_block(w, c0, nb, u, elem)


@gptq_mx_block.register_fake
def _(w, c0, nb, u, elem):
    return w.new_empty((w.shape[0], nb), dtype=torch.float32), w.new_empty((w.shape[0], -(-w.shape[1] // ops.MX_BLOCK)), dtype=torch.uint8)


@torch.library.custom_op("dipoorlet::fake_quant_set", mutates_args=(), device_types="cuda")
def fake_quant_set(xs: List[torch.Tensor], scales: List[torch.Tensor], zero_points: List[torch.Tensor], inner: List[int],
                   qlo: List[int], qhi: List[int]) -> List[torch.Tensor]:
    """Fused Q -> DQ of every tensor of a batch in ONE launch (dpl_fake_quant_items).  scales[t] / zero_points[t]: [1] or [C] (fp32 /
    int32 device tensors — kept by the cached plan: pass the same tensors on every call); inner[t]: elements behind the channel
    axis of tensors[t] as laid out in memory (ignored per tensor)."""
    xs = _contig(xs)
    c = _cached(xs, 1)
    key = (tuple(s.data_ptr() for s in scales), tuple(z.data_ptr() for z in zero_points), tuple(inner), tuple(qlo), tuple(qhi))
    fq = c.fq.get(key)
    if fq is None:
        if len(c.fq) >= 8:
            c.fq.pop(next(iter(c.fq)))
        fq = c.fq[key] = ops.FakeQuantSet(c.plan, list(zip(scales, zero_points, inner, qlo, qhi)))
    return fq(xs)


@fake_quant_set.register_fake
def _(xs, scales, zero_points, inner, qlo, qhi):
    return [torch.empty_like(x, memory_format=torch.contiguous_format) for x in xs]
