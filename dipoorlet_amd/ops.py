"""Torch-facing operators over the C ABI: device memory and streams come from PyTorch-ROCm, the
arithmetic runs in the hand-written gfx950 kernels (csrc/*.hip; the statistics chain: csrc/calib_kernels.hip).

Vocabulary: a *tensor set* is the list of activation tensors one forward of the network yields for a
batch of B calibration images (each tensor is [B, ...] contiguous fp32).  A `TensorSetPlan` cuts the
set into work items once; `CalibAccumulators` holds the persistent device-side statistics
(running min/max, uint64 histograms, OCTAV states) that replace the reference's per-image Python
lists (forward_net.py:204-235, 252-280, 297-340).
"""
import collections
import ctypes as C
import os
import weakref

import numpy as np
import torch

from . import _hip

_SEG_CACHE_MAX = 64


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _require_cuda(t, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise _hip.DipoorletHipError(f"{name} must be a ROCm device tensor; dipoorlet_amd has no CPU path")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _hip.DipoorletHipError(f"{name} must be contiguous float32")


def _upload_struct_array(arr, n, device):
    """ctypes struct array -> device uint8 tensor (one-off, synchronous)."""
    nbytes = C.sizeof(arr._type_) * max(n, 1)
    host = torch.frombuffer(bytearray(C.string_at(C.addressof(arr), nbytes)), dtype=torch.uint8)
    return host.to(device)


# Workgroups per launch for the balanced partition (tuned on MI355X: few, large, equal shares stream
# faster from HBM than many small items; the histogram wants a little more latency hiding).
DEFAULT_BLOCKS = {"minmax": 256, "hist": 768, "octav": 1024, "cos": 512, "fq": 65536}   # measured optima per kernel family


class WorkSet:
    """Device-resident work decomposition of one launch: items (+ block_begin for the balanced form)."""

    def __init__(self, items, n_items, block_begin, n_blocks):
        self.items, self.n_items, self.block_begin, self.n_blocks = items, n_items, block_begin, n_blocks

    def args(self):
        """(d_items, n_items, d_block_begin, n_blocks) as the C ABI takes them."""
        bb = _ptr(self.block_begin) if self.block_begin is not None else C.c_void_p(0)
        return _ptr(self.items), self.n_items, bb, self.n_blocks


class TensorSetPlan:
    """Static decomposition of a tensor set into work.

    elems_per_image[t] = elements of tensor t for ONE image; batch = images stacked along dim 0.
    Slots: tensor index t (per_image=False: images of a batch merge for free) or b * T + t (per image).
    Default form: the balanced partition (dpl_build_balanced_items) with a per-kernel workgroup count.
    chunk_elems forces the one-item-per-workgroup form (dpl_build_work_items) instead.
    """

    def __init__(self, elems_per_image, batch, device, chunk_elems=None):
        self.elems = [int(e) for e in elems_per_image]
        self.batch = int(batch)
        self.T = len(self.elems)
        self.device = torch.device(device)
        self.total = sum(self.elems) * self.batch
        self.chunk = int(chunk_elems) if chunk_elems else None
        self._work = {}
        self._elems_dev = None      # filled by elems_device(): the plan's first range pass
        self._octav_scratch = None  # ... by octav_scratch()
        self._octav_lh = None       # ... by octav_loghist_scratch()
        self._octav_tail = None     # ... by octav_tail(): the OctavTailPlan, or False where the C ABI refuses the set
        self._octav_rotations = weakref.WeakSet()   # every pipeline's _Rotation on this plan
        self._seg_cache = {}        # seg_table(): pointer tuple -> slot of the block the first launch allocates:
        self._seg_dev = self._seg_host = self._seg_np = None    # [slots, T] int64: device, pinned, the pinned one as numpy
        self._seg_copied = self._seg_keys = None    # per slot: the event behind its last upload, its pointer tuple
        self._seg_next = 0

    @property
    def n_pairs(self):
        return self.batch * self.T

    def _spans(self, per_image):
        if per_image:
            return [(t, b * e, e, b * self.T + t) for b in range(self.batch) for t, e in enumerate(self.elems)]
        return [(t, 0, e * self.batch, t) for t, e in enumerate(self.elems)]

    def work(self, kind, per_image=False):
        """WorkSet for kernel family `kind` in {'minmax', 'hist', 'octav', 'cos', 'fq'}."""
        nb = None if self.chunk else max(1, min(DEFAULT_BLOCKS[kind], (self.total + 4095) // 4096))
        key = (per_image, nb)
        w = self._work.get(key)
        if w is None:
            spans = self._spans(per_image)
            if self.chunk:
                arr, n = _hip.build_work_items(spans, self.chunk)
                w = WorkSet(_upload_struct_array(arr, n, self.device), n, None, n)
            else:
                arr, n, bb = _hip.build_balanced_items(spans, nb)
                bbt = torch.frombuffer(bytearray(bytes(bb)), dtype=torch.int32).to(self.device)
                w = WorkSet(_upload_struct_array(arr, n, self.device), n, bbt, nb)
            self._work[key] = w
        return w

    def elems_device(self):
        """uint64 [T] on the device: elements of every tensor of a batch (what dpl_hist_spec_accumulate partitions).  Uploaded once
        per plan, synchronously, like the work sets: a plan's first range pass waits for that copy, no later call does."""
        if self._elems_dev is None:
            self._elems_dev = torch.tensor([e * self.batch for e in self.elems], dtype=torch.int64, device=self.device)
        return self._elems_dev

    def octav_scratch(self):
        """(pair_spans, pair_base u64 [B*T], pair_order, list0, list1): where each pair's data lives, and two tail lists of
        the batch's size with the pair regions laid out in pair order (32-element aligned: whole 128-byte lines)."""
        if self._octav_scratch is None:
            # (a region starts on a 128-byte line: the streaming workgroup that walks a pair reads back the list it has just
            # written, and no other workgroup of the launch may have pulled a line of it into the CU's L1 beforehand — which a
            # neighbouring pair's last, straddling line would)
            sizes = [((e + 31) // 32) * 32 for _ in range(self.batch) for e in self.elems]
            base = np.zeros(len(sizes) + 1, np.int64)       # (n + 1 entries: a region's size is the difference of two)
            base[1:] = np.cumsum(sizes)
            tot = int(sum(sizes))
            arr, ns = _hip._span_array(self._spans(True))
            order = np.argsort(-np.array(sizes, np.int64), kind="stable").astype(np.int32)  # largest pairs first
            self._octav_scratch = (_upload_struct_array(arr, ns, self.device), torch.from_numpy(base).to(self.device),
                                   torch.from_numpy(order).to(self.device),
                                   torch.empty(tot, dtype=torch.float32, device=self.device),
                                   torch.empty(tot, dtype=torch.float32, device=self.device))
        return self._octav_scratch

    def octav_loghist_scratch(self):
        """(count u32 [B*T, 2048], mantissa-sum u64 [B*T, 2048], bitmap u32 [B*T, 66]) for the bracket form."""
        if self._octav_lh is None:
            n = self.n_pairs
            self._octav_lh = (torch.empty(n, 2048, dtype=torch.int32, device=self.device),
                              torch.empty(n, 2048, dtype=torch.int64, device=self.device),
                              torch.empty(n, 66, dtype=torch.int32, device=self.device))
        return self._octav_lh

    def octav_tail(self):
        """The exact-tail form's HOST plan (dpl_octav_plan_*: every buffer size comes from the C ABI), its static tables on the
        device and the threshold history of this tensor set — or None when a pair needs more than 64 slices."""
        if self._octav_tail is None:
            arr, ns = _hip._span_array(self._spans(True))
            L = _hip.lib()
            handle = L.dpl_octav_plan_create(C.addressof(arr), ns, self.T, max(1, min(DEFAULT_BLOCKS["octav"], (self.total + 4095) // 4096)))
            self._octav_tail = OctavTailPlan(self, handle) if handle else False
        return self._octav_tail or None

    def octav_reset(self):
        """Cold start of the exact-tail OCTAV form: what the plan learned from earlier batches (the thresholds its tensors' pairs
        asked for) is forgotten — the state of a plan that has never run.  Call between independent calibration runs that share
        a plan (after OctavPipeline.sync())."""
        rotations = list(self._octav_rotations)
        if any(st.pending for rot in rotations for st in rot.sets):    # (asked of every pipeline before anything changes)
            raise _hip.DipoorletHipError("octav_reset with batches in flight: call OctavPipeline.sync() first")
        if self._octav_tail:
            self._octav_tail.history.zero_()
            self._octav_tail.calls = 0
        for rot in rotations:
            rot.restart()

    def _validate(self, tensors):
        if len(tensors) != self.T:
            raise _hip.DipoorletHipError(f"expected {self.T} tensors, got {len(tensors)}")
        for t, (x, e) in enumerate(zip(tensors, self.elems)):
            _require_cuda(x, f"tensor {t}")
            if x.numel() != e * self.batch:
                raise _hip.DipoorletHipError(f"tensor {t}: {x.numel()} elements, plan expects {e * self.batch}")

    def bind(self, tensors):
        """A tensor set a caller keeps RESIDENT and launches over again and again (pass 2 of `-A hist`, bench.py's pools):
        validated once, then held — the BoundSet owns references to the tensors, so their memory cannot be handed to another
        tensor while it lives, and a launch over it costs no per-tensor checks (557 tensors of a ViT-B/16 set: 0.1 - 0.2 ms of
        host time per launch otherwise, more than the host has to spare per batch).

        CONTRACT: the contents of a bound set are taken as UNCHANGED between its range pass (CalibAccumulators.minmax_accumulate)
        and its histogram pass (abs_hist_accumulate) on one accumulator: the range pass already histograms the set against the
        running range, and the histogram pass does not read a tensor again whose guess turned out right.  A caller that rewrites
        bound tensors in place between the two builds its accumulator with speculate=False."""
        if isinstance(tensors, BoundSet):
            if tensors.plan is not self:
                raise _hip.DipoorletHipError("this tensor set is bound to another plan")
            return tensors
        tensors = list(tensors)
        self._validate(tensors)
        host = torch.tensor([x.data_ptr() for x in tensors], dtype=torch.int64).pin_memory()
        return BoundSet(self, tensors, host.to(self.device, non_blocking=True), host)

    def seg_table(self, tensors):
        """Device table of base pointers for this launch.  A list of tensors is checked on EVERY call (device, dtype, contiguity,
        element count: the allocator hands a freed set's addresses to other tensors, so a pointer seen before proves nothing);
        the table itself is cached per pointer tuple.  A BoundSet (bind()) was checked when it was bound.

        The tables live in ONE block allocated with the plan's first launch — _SEG_CACHE_MAX slots of T pointers on the device and
        the same in pinned host memory: a pointer tuple not seen before takes the next slot in rotation (written on the host,
        copied asynchronously on the current stream), so a launch over new tensors allocates nothing and does not wait for the
        device.  A slot is rewritten _SEG_CACHE_MAX distinct tensor sets later; no launch of this library is that far behind the
        host (the OCTAV pipeline runs at most DPL_OCTAV_PIPE_SETS batches ahead)."""
        if isinstance(tensors, BoundSet):
            if tensors.plan is not self:
                raise _hip.DipoorletHipError("this tensor set is bound to another plan")
            return tensors.table
        self._validate(tensors)
        key = tuple(x.data_ptr() for x in tensors)
        slot = self._seg_cache.get(key)
        if slot is not None:
            return self._seg_dev[slot]
        if self._seg_dev is None:
            self._seg_host = torch.empty(_SEG_CACHE_MAX, max(self.T, 1), dtype=torch.int64).pin_memory()
            self._seg_np = self._seg_host.numpy()
            self._seg_dev = torch.empty(_SEG_CACHE_MAX, max(self.T, 1), dtype=torch.int64, device=self.device)
            self._seg_copied = [None] * _SEG_CACHE_MAX
            self._seg_keys = [None] * _SEG_CACHE_MAX
        slot = self._seg_next % _SEG_CACHE_MAX
        self._seg_next += 1
        self._seg_cache.pop(self._seg_keys[slot], None)
        ev = self._seg_copied[slot]
        if ev is not None and not ev.query():       # (the copy that last read this pinned row has not run yet: 64 sets ago)
            ev.synchronize()
        self._seg_np[slot, :len(key)] = key
        self._seg_dev[slot].copy_(self._seg_host[slot], non_blocking=True)
        self._seg_copied[slot] = torch.cuda.current_stream(self.device).record_event(ev)
        self._seg_keys[slot] = key
        self._seg_cache[key] = slot
        return self._seg_dev[slot]


class OctavTailPlan:
    """dpl_octav_plan of one TensorSetPlan: sizes, tables, history, and the buffers of the single-stream use (octav_batch)."""

    def __init__(self, plan, handle):
        # (what it needs of the TensorSetPlan that owns it, not the plan itself: a reference back would tie the two into a cycle,
        # and a dropped plan's workspace — tens of MB per tensor set — would wait for the cycle collector instead of going at once)
        self.device, self.n_pairs, self.handle = plan.device, plan.n_pairs, handle
        L = _hip.lib()
        self.sizes = _hip.OctavWorkspaceSizes()
        _hip.check(L.dpl_octav_plan_sizes(handle, C.byref(self.sizes)), "dpl_octav_plan_sizes")
        dev = plan.device
        self.tables = torch.empty(int(self.sizes.tables_bytes), dtype=torch.uint8, device=dev)
        # (no synchronisation here: the copies' sources are the C plan's own host tables, which live as long as this object —
        # __del__ waits for this event before it lets go of them)
        _hip.check(L.dpl_octav_plan_upload(handle, _ptr(self.tables), _stream()), "dpl_octav_plan_upload")
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(torch.cuda.current_stream(dev))
        self.history = torch.zeros(int(self.sizes.history_bytes), dtype=torch.uint8, device=dev)
        self.calls = 0          # batches run on this history through octav_batch (pipelines count their own)
        self.n_multi = int(self.sizes.n_multi)
        self._single = None     # (state, rescue, list0, list1) of octav_batch
        self.fallback = None    # the compaction route's lists: allocated when a batch first reports unfinished pairs
        self.fallback_block = None  # ... whole-batch ones, bound to every job of octav_batch(inline=True): allocated by its first call

    def __del__(self):
        try:
            self._uploaded.synchronize()
            _hip.lib().dpl_octav_plan_destroy(self.handle)
        except Exception:   # noqa: BLE001  (interpreter shutdown)
            pass

    def new(self, what):
        """A device buffer of the workspace part `what` ('state', 'rescue', 'list', 'fallback', 'result')."""
        n = int(getattr(self.sizes, what + "_bytes"))
        return torch.empty(max(n, 256), dtype=torch.uint8, device=self.device)

    def compaction(self, job, states, stream, arena=None, host_states=None, base_host=None):
        """The compaction route for the pairs of `job`'s batch that neither their walk nor the rescue finished (its control block
        said so; rare — flat distributions, values beyond 2^14, lists beyond their regions, a dozen pairs of a cold first batch):
        dpl_octav_fallback_layout gives regions to just those pairs, and the route's two lists are that small (arena: a buffer to
        reuse; returned, grown if need be).
        host_states: the batch's states in PINNED host memory, already valid (the pipeline copies them behind every batch's rescue
        and reads them when the set comes up for reuse) — nothing here waits for the device then; without it the states are read
        back now (one host synchronisation on `stream`: octav_batch).  base_host: a pinned buffer of 8 (n_pairs + 1) bytes for the
        region table's upload (same rule)."""
        L = _hip.lib()
        n = self.n_pairs
        if host_states is None:
            with torch.cuda.stream(stream):
                host_states = states[:(n + 1) * C.sizeof(_hip.OctavState)].cpu()
        if base_host is None:
            base = np.zeros(n + 1, np.uint64)
        else:
            base = base_host.numpy().view(np.uint64)[:n + 1]
        total = int(L.dpl_octav_fallback_layout(host_states.data_ptr(), n, base.ctypes.data))
        if total < 0:
            _hip.check(total, "dpl_octav_fallback_layout")
        if total == 0:
            return arena
        with torch.cuda.stream(stream):
            need = 2 * 4 * total + 8 * (n + 1)
            if arena is None or arena.numel() < need:
                arena = torch.empty(need + need // 2, dtype=torch.uint8, device=self.device)
            tab = arena[2 * 4 * total:2 * 4 * total + 8 * (n + 1)]
            if base_host is None:
                tab.copy_(torch.from_numpy(base.view(np.uint8)))       # (a blocking copy of 8 (n + 1) bytes)
            else:
                tab.copy_(base_host[:8 * (n + 1)], non_blocking=True)
        job.d_pair_base_full = tab.data_ptr()
        job.d_clist0 = arena.data_ptr()
        job.d_clist1 = arena.data_ptr() + 4 * total
        _hip.check(L.dpl_octav_oneread_compaction(C.byref(job), C.c_void_p(stream.cuda_stream)), "dpl_octav_oneread_compaction")
        return arena

    def bind(self, state, rescue, list0, list1, tab, call_index, dyn, fallback=None):
        j = _hip.OctavOnereadJob()
        _hip.check(_hip.lib().dpl_octav_plan_bind(self.handle, _ptr(self.tables), _ptr(self.history), _ptr(state), _ptr(rescue),
                                                  _ptr(list0), _ptr(list1), _ptr(fallback) if fallback is not None else None,
                                                  _ptr(tab), int(call_index), dyn, _OCTAV_MAX_ITERS, C.byref(j)), "dpl_octav_plan_bind")
        return j

    def single(self):
        if self._single is None:
            self._single = (self.new("state"), self.new("rescue"), self.new("list"), self.new("list"))
        return self._single


class BoundSet:
    """A validated, resident tensor set of one plan (TensorSetPlan.bind): the tensors, kept alive, and their device pointer
    table.  Accepted wherever a list of the set's tensors is."""
    __slots__ = ("plan", "tensors", "table", "_host", "__weakref__")   # (weakly referenced by CalibAccumulators' ledger)

    def __init__(self, plan, tensors, table, host):
        self.plan, self.tensors, self.table, self._host = plan, tensors, table, host

    def __len__(self):
        return len(self.tensors)

    def __iter__(self):
        return iter(self.tensors)

    def __getitem__(self, i):
        return self.tensors[i]


class _LedgerRecord(collections.namedtuple("_LedgerRecord", "ref entry T")):
    """CalibAccumulators' ledger: a bound set (weakly), its slab entry, the T slots the entry is laid out for (read by name
    here; still a tuple, because tests/test_hist_spec_gpu.py reads the entry by position)."""
    __slots__ = ()


def qmse_grid(qtype, bit_width=8):
    """(grid, top) of dpl_hist_qmse for a platform's qi_params["type"]: "Linear" — the integers up to 2 ** (bit_width - 1) - 1,
    quantize._symmetric_grid's — or "Float8E4M3FN" (the format's own codes: top is not an argument)."""
    if qtype == "Linear":
        return _hip.GRID_UNIFORM, 2 ** (int(bit_width) - 1) - 1
    if qtype == "Float8E4M3FN":
        return _hip.GRID_E4M3, 0
    raise _hip.DipoorletHipError(f"hist_qmse: no grid for quantisation type {qtype!r} (Linear or Float8E4M3FN)")


class CalibAccumulators:
    """Persistent per-tensor statistics on the device.

    speculate=True: the range pass over a BoundSet (per_image=False) also histograms the batch, against the range the running
    min / max give before that launch, into a ledger entry of this accumulator ([T, bins] uint32 counts per bound set); the
    histogram pass over the same BoundSet adds the rows whose guessed range turned out to be the final one — byte for byte, so the
    counts are the ones a second read would give — and reads only the other tensors (dpl_hist_spec_accumulate).  A running
    dmax stops moving once the batch that holds the tensor's extreme has passed, so about half of all (batch, tensor) pairs of a
    shard need no second read.  The contents of a bound set must not change between the two passes (TensorSetPlan.bind);
    speculate=False for a caller that rewrites bound tensors in place.

    The ledger: one entry per bound set (a later range pass over the same set overwrites it), emptied by reset_minmax(), left
    alone by set_minmax / hist_prepare (merged ranges decide by the same byte comparison).  Entries come from a slab this object
    holds for its lifetime and reuses — after the first sweep a call allocates nothing, and after a plan's first range pass (which
    uploads the plan's work set and element counts once) none waits for the device — and the ledger refers to a bound set
    weakly: dropping the set frees its tensors.  A plan does not speculate when an entry (T * bins * 4 bytes) would exceed
    1 / SPEC_MAX_SHARE of the batch's bytes (the zeroing and the flush of the entry would no longer be small against the read),
    when a tensor of the batch has 2^32 elements or more (uint32 counts), above _hip.HIST_SPEC_MAX_TENSORS tensors, or in the
    chunk_elems form: it then runs the plain range pass.  spec_stats() / spec_flags() say what was skipped."""

    SPEC_MAX_SHARE = 64     # an entry may take at most 1/64 of the bytes of the batch it describes

    def __init__(self, n_slots, device, bins=2048, speculate=True):
        self.n = int(n_slots)
        self.device = torch.device(device)
        self.bins = int(bins)
        if not (1 <= self.bins <= _hip.MAX_BINS):
            raise _hip.DipoorletHipError(f"bins must be in [1, {_hip.MAX_BINS}]")
        self.min_enc = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self.max_enc = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self.nan = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self.gmin = torch.empty(self.n, dtype=torch.float32, device=self.device)
        self.gmax = torch.empty(self.n, dtype=torch.float32, device=self.device)
        self.hist = None
        self.ranges = None
        self.speculate = bool(speculate)
        self._ledger = {}       # id(bound set) -> _LedgerRecord
        self._slab = []         # entries not in use: held for this object's lifetime, never returned to the allocator in between
        self._spec_stats = torch.zeros(4, dtype=torch.int64, device=self.device) if self.speculate else None
        self.reset_minmax()

    def reset_minmax(self):
        """Running min / max back to 'no data'; the ledger of range-pass histograms is emptied (its entries go back to the slab)."""
        self._slab.extend(rec.entry for rec in self._ledger.values())
        self._ledger.clear()
        _hip.check(_hip.lib().dpl_minmax_init(_ptr(self.min_enc), _ptr(self.max_enc), _ptr(self.nan), self.n,
                                              _stream()), "dpl_minmax_init")

    # ---- the ledger
    def will_speculate(self, plan, tensors, per_image=False):
        """Whether minmax_accumulate(plan, tensors, per_image) takes the fused path (the class docstring gives the conditions)."""
        return (self.speculate and isinstance(tensors, BoundSet) and not per_image and plan.chunk is None
                and 0 < plan.T <= min(self.n, _hip.HIST_SPEC_MAX_TENSORS)
                and max(plan.elems) * plan.batch < (1 << 32)
                and plan.T * self.bins * 4 * self.SPEC_MAX_SHARE <= plan.total * 4)

    def _live(self, bound):     # the live record of this bound set, or None (an id may outlive its set)
        rec = self._ledger.get(id(bound))
        return rec if rec is not None and rec.ref() is bound else None

    def _entry_for(self, bound):
        rec = self._live(bound)
        if rec is not None:
            return rec.entry
        # (An entry may be used on another stream than the one current when it was allocated: the CLI's range pass runs on a side
        # stream, its histogram pass on the caller's, ordered by main.wait_stream(side).  That is safe because the slab holds every
        # entry for this object's lifetime — no block goes back to the allocator while work on either stream may still be queued;
        # whoever lets an accumulator go right behind a histogram pass must synchronise first, as reading acc.hist does.)
        if self._slab:
            entry = self._slab.pop()
        else:
            nbytes = int(_hip.lib().dpl_hist_spec_entry_bytes(self.n, self.bins))
            entry = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        key, slab, ledger = id(bound), self._slab, self._ledger

        def dropped(ref):           # the bound set died: its entry is free again (the ledger never kept the set alive)
            rec = ledger.get(key)
            if rec is not None and rec.ref is ref:     # (the set is gone: the record must still be its own)
                del ledger[key]
                slab.append(rec.entry)
        self._ledger[key] = _LedgerRecord(weakref.ref(bound, dropped), entry, bound.plan.T)
        return entry

    def _entry_of(self, plan, tensors):
        rec = self._live(tensors) if isinstance(tensors, BoundSet) else None
        return rec.entry if rec is not None and rec.T == plan.T else None

    def spec_stats(self, reset=False):
        """HOST (synchronises): what the histogram passes so far skipped — {'pairs', 'pairs_skipped', 'elements',
        'elements_skipped'} over the (batch, tensor) pairs of every abs_hist_accumulate call that found a ledger entry."""
        v = [0, 0, 0, 0] if self._spec_stats is None else [int(x) for x in self._spec_stats.cpu().tolist()]
        if reset and self._spec_stats is not None:
            self._spec_stats.zero_()
        return dict(zip(("pairs", "pairs_skipped", "elements", "elements_skipped"), v))

    def spec_flags(self, tensors):
        """HOST (synchronises): per tensor what the last abs_hist_accumulate over this bound set did — 1: the range pass's row was
        added and the tensor not read, 2: nothing to count (range status != 0), 0: read — or None when the set has no entry."""
        rec = self._live(tensors)
        if rec is None:
            return None
        off = rec.T * C.sizeof(_hip.HistRange)      # (the entry is laid out for the T slots of the set's plan: dpl_hist_spec_entry_bytes)
        return rec.entry[off:off + 4 * rec.T].view(torch.int32).cpu()

    def spec_cuts(self, plan, tensors):
        """HOST (synchronises; a test hook): the n_blocks + 1 cuts the histogram pass's kernel works to for the flags this bound
        set's entry holds now, as positions in the stream of the tensors still to be read (tests/hist_spec_model.py: cuts)."""
        entry = self._entry_of(plan, tensors)
        if entry is None:
            return None
        nb = plan.work("hist").n_blocks
        out = torch.empty(nb + 1, dtype=torch.int64, device=self.device)
        _hip.check(_hip.lib().dpl_hist_spec_cuts(_ptr(entry), _ptr(plan.elems_device()), plan.T, nb, _ptr(out), _stream()),
                   "dpl_hist_spec_cuts")
        return out.cpu()

    # ---- pass 1
    def minmax_accumulate(self, plan, tensors, per_image=False):
        """per_image=False: slot = tensor (n_slots = T).  per_image=True: slot = image * T + tensor
        (n_slots = B * T), the reference's one-entry-per-image lists.
        A BoundSet with per_image=False also leaves the batch's histogram against the running range in the ledger (speculate)."""
        tab = plan.seg_table(tensors)
        if self.n < (plan.n_pairs if per_image else plan.T):
            raise _hip.DipoorletHipError("accumulator has fewer slots than the plan addresses")
        if self.will_speculate(plan, tensors, per_image):
            w = plan.work("hist")
            entry = self._entry_for(tensors)
            plan.elems_device()     # (uploaded with the plan's first range pass, not in the middle of the histogram pass)
            _hip.check(_hip.lib().dpl_minmax_hist_accumulate(*w.args(), _ptr(tab), _ptr(self.min_enc), _ptr(self.max_enc),
                                                             _ptr(self.nan), plan.T, self.bins, _ptr(entry), _stream()),
                       "dpl_minmax_hist_accumulate")
            return
        if isinstance(tensors, BoundSet):       # (a plain range pass over a set that has an entry: the entry no longer describes it)
            rec = self._live(tensors)
            if rec is not None:
                del self._ledger[id(tensors)]
                self._slab.append(rec.entry)
        w = plan.work("minmax", per_image)
        _hip.check(_hip.lib().dpl_minmax_accumulate(*w.args(), _ptr(tab), _ptr(self.min_enc), _ptr(self.max_enc),
                                                    _ptr(self.nan), _stream()), "dpl_minmax_accumulate")

    def finalize_minmax(self):
        """-> (gmin, gmax) fp32 device tensors [n_slots]."""
        _hip.check(_hip.lib().dpl_minmax_finalize(_ptr(self.min_enc), _ptr(self.max_enc), _ptr(self.nan), self.n,
                                                  _ptr(self.gmin), _ptr(self.gmax), _stream()),
                   "dpl_minmax_finalize")
        return self.gmin, self.gmax

    def set_minmax(self, gmin, gmax):
        """Install merged ranges (e.g. after an all-reduce across ranks)."""
        self.gmin.copy_(gmin)
        self.gmax.copy_(gmax)
        _hip.check(_hip.lib().dpl_minmax_encode(_ptr(self.gmin), _ptr(self.gmax), self.n, _ptr(self.min_enc),
                                                _ptr(self.max_enc), _ptr(self.nan), _stream()), "dpl_minmax_encode")

    # ---- pass 2
    def hist_prepare(self):
        """Derive per-tensor histogram ranges from gmin/gmax (call after finalize_minmax / set_minmax)."""
        if self.hist is None:
            self.hist = torch.zeros(self.n, self.bins, dtype=torch.int64, device=self.device)
            self.ranges = torch.empty(self.n * C.sizeof(_hip.HistRange), dtype=torch.uint8, device=self.device)
        else:
            self.hist.zero_()
        _hip.check(_hip.lib().dpl_hist_prepare(_ptr(self.gmin), _ptr(self.gmax), self.n, self.bins,
                                               _ptr(self.ranges), _stream()), "dpl_hist_prepare")

    def abs_hist_accumulate(self, plan, tensors):
        """hist += the |x| histogram of this batch.  A BoundSet whose range pass left a ledger entry is read only where the entry's
        guessed range is not the final one (the same counts either way)."""
        tab = plan.seg_table(tensors)
        w = plan.work("hist")
        entry = self._entry_of(plan, tensors)
        if entry is not None:
            _hip.check(_hip.lib().dpl_hist_spec_accumulate(_ptr(entry), _ptr(plan.elems_device()), plan.T, w.n_blocks, _ptr(tab),
                                                           _ptr(self.ranges), self.bins, _ptr(self.hist), _ptr(self._spec_stats),
                                                           _stream()), "dpl_hist_spec_accumulate")
            return
        _hip.check(_hip.lib().dpl_abs_hist_accumulate(*w.args(), _ptr(tab), _ptr(self.ranges), self.bins,
                                                      _ptr(self.hist), _stream()), "dpl_abs_hist_accumulate")

    def range_status(self):
        """HOST (synchronises): per-slot status from dpl_hist_prepare: 0 ok, 1 not finite, 2 too many bins."""
        raw = self.ranges.cpu().numpy().view(np.dtype([("first", "<f4"), ("last", "<f4"), ("step", "<f4"),
                                                       ("inv", "<f4"), ("zero_bin", "<u4"), ("status", "<u4"),
                                                       ("dmax", "<f4"), ("exact_div", "<u4")]))
        return raw

    def hist_percentile(self, threshold):
        clip = torch.empty(self.n, 2, dtype=torch.float32, device=self.device)
        _hip.check(_hip.lib().dpl_hist_percentile(_ptr(self.hist), _ptr(self.gmin), _ptr(self.gmax), self.n,
                                                  self.bins, float(threshold), _ptr(clip), _stream()),
                   "dpl_hist_percentile")
        return clip

    def hist_kl(self, levels):
        """Entropy (KL-divergence) clip search on the accumulated histograms (k_hist_kl; the definition: tests/kl_model.py)
        -> (clip [n, 2] fp32, best [n] int32: the number of bins kept, -1 where no candidate is admissible and the clip is the
        range, div [n, bins + 1] fp64: every candidate's divergence, +inf where not admissible or below `levels`)."""
        levels = int(levels)
        if not (2 <= levels <= self.bins):
            raise _hip.DipoorletHipError(f"hist_kl: levels must be in [2, bins = {self.bins}], got {levels}")
        clip = torch.empty(self.n, 2, dtype=torch.float32, device=self.device)
        best = torch.empty(self.n, dtype=torch.int32, device=self.device)
        div = torch.empty(self.n, self.bins + 1, dtype=torch.float64, device=self.device)
        _hip.check(_hip.lib().dpl_hist_kl(_ptr(self.hist), _ptr(self.gmin), _ptr(self.gmax), self.n, self.bins, levels,
                                          _ptr(div), _ptr(best), _ptr(clip), _stream()), "dpl_hist_kl")
        return clip, best, div

    def hist_qmse(self, qtype, bit_width=8, first=128):
        """Quantisation-MSE clip search on the accumulated histograms (k_hist_qmse; the definition: tests/qmse_model.py): the
        bin centres fake-quantised on the grid of `qtype` (a platform's qi_params["type"]: "Linear" — the integers up to
        2 ** (bit_width - 1) - 1 — or "Float8E4M3FN") for every candidate "keep `i` bins", i in [first, bins]
        -> (clip [n, 2] fp32, best [n] int32: the bins kept, -1 for an empty histogram, whose clip is the range,
        err [n, bins + 1] fp64: every candidate's mean squared error in bin widths^2, +inf below `first`)."""
        grid, top = qmse_grid(qtype, bit_width)
        clip = torch.empty(self.n, 2, dtype=torch.float32, device=self.device)
        best = torch.empty(self.n, dtype=torch.int32, device=self.device)
        err = torch.empty(self.n, self.bins + 1, dtype=torch.float64, device=self.device)
        _hip.check(_hip.lib().dpl_hist_qmse(_ptr(self.hist), _ptr(self.gmin), _ptr(self.gmax), self.n, self.bins, int(first), grid, top,
                                            _ptr(err), _ptr(best), _ptr(clip), _stream()), "dpl_hist_qmse")
        return clip, best, err


_OCTAV_MAX_ITERS = 20  # forward_net.py:325


_OCTAV_MODE = {"full": 0, "compact": 1, "bracket": 2, "tail": 3}
_ONEREAD_EPOCH = 8      # batches per threshold-history epoch (the C ABI's: dpl_octav_plan_bind); a batch lists by what the
                        # pairs of the current and the previous epoch asked for (8 - 16 batches of history)


def _default_form():
    """DPL_OCTAV_FORM, else 'tail' (exact tail / bounded bulk; csrc/octav_tail.hpp)."""
    form = os.environ.get("DPL_OCTAV_FORM", "tail")
    if form not in _OCTAV_MODE:
        raise _hip.DipoorletHipError(f"DPL_OCTAV_FORM={form}: the forms are {sorted(_OCTAV_MODE)}")
    return form


def octav_batch(plan, tensors, dynamic_sym, states=None, form=None, inline=False):
    """OCTAV for every (image, tensor) pair of one batch -> fp32 device tensor [B, T, 3] = (s, min, max).

    Forms (all end on the reference's result, forward_net.py:323-330):
      'tail' (default)     ONE read, one launch: statistics, exact log-scale histogram and the values at or above a threshold
                           bin (~1 % of a pair); the early iterates are taken as lower bounds from the histogram, the late
                           ones exactly from the list; a walk that does not end on two exact evaluations is rescued by the
                           exact two-read route (csrc/octav_tail.hpp).  Pairs of up to 64 slices (a pair above one slice —
                           dpl_octav_slice_cap() elements — is streamed slice by slice and walked by a merge kernel; a set with
                           a larger pair runs 'bracket'); every buffer is sized by the C ABI (dpl_octav_plan_*, OctavTailPlan).
                           This call reads the batch's control block back (one host synchronisation); OctavPipeline defers that;
                           inline=True runs the compaction route inline instead, on a whole-batch fallback block (OctavTailPlan.
                           fallback_block: 8 bytes per element of the batch, allocated by the plan's first such call) — no host
                           synchronisation, the rows final in stream order (the custom ops, torch_ops.py)
      'bracket'            two reads: statistics + exact log-scale histogram, bracket walk, gather of the marked
                           bins, exact per-pair iteration; pairs it cannot serve finish on the compaction route
      'compact'            evaluation at s_0 + tail compaction, then per-pair iteration over shrinking lists
      'full'               every evaluation re-reads the full data (21 passes)
    DPL_OCTAV_FORM overrides the default.
    Tolerance: every form is within 1e-5 * max(1, |ref|) of the reference's optimal_s (the tests' bound; the reference's own stop
    rule is an absolute 1e-6); min / max are exact.  'tail' repeats to about 1e-6 relative from run to run, not bit for bit — the
    threshold history and wave timing decide which early iterates are taken as bounds, and with them the iterate on which
    |s' - s| < 1e-6 fires — while 'bracket' walks the reference's whole iterate sequence over exact integer sums and is bit-stable
    (the exact fall-back, and the reference point of the golden tests).
    states (optional): a uint8 device buffer of (B * T + 1) * 80 bytes that receives the pairs' states and the control block."""
    if form is None:
        form = _default_form()
    mode = _OCTAV_MODE[form]
    if form == "tail":
        tp = plan.octav_tail()
        if tp is not None:
            return _octav_batch_tail(plan, tp, tensors, dynamic_sym, states, inline)
        mode = 2            # a pair above 64 slices: the two-read form
    w = plan.work("octav", per_image=True)
    n_pairs = plan.n_pairs
    nbytes = (n_pairs + 1) * C.sizeof(_hip.OctavState)  # + control block
    if states is None or states.numel() < nbytes:
        states = torch.empty(nbytes, dtype=torch.uint8, device=plan.device)
    tab = plan.seg_table(tensors)
    L = _hip.lib()
    dyn = 1 if dynamic_sym else 0
    _hip.check(L.dpl_octav_init(_ptr(states), n_pairs, mode, _stream()), "dpl_octav_init")
    if mode == 0:
        _hip.check(L.dpl_octav_run(*w.args(), _ptr(tab), _ptr(states), n_pairs, dyn, _OCTAV_MAX_ITERS, _stream()),
                   "dpl_octav_run")
    else:
        spans, base, order, l0, l1 = plan.octav_scratch()
        if mode == 1:
            _hip.check(L.dpl_octav_run_compact(*w.args(), _ptr(tab), _ptr(states), n_pairs, _ptr(spans), _ptr(base),
                                               _ptr(order), _ptr(l0), _ptr(l1), dyn, _OCTAV_MAX_ITERS, _stream()),
                       "dpl_octav_run_compact")
        else:
            cnt, msum, bitmap = plan.octav_loghist_scratch()
            _hip.check(L.dpl_octav_run_bracket(*w.args(), _ptr(tab), _ptr(states), n_pairs, _ptr(spans), _ptr(base),
                                               _ptr(order), _ptr(l0), _ptr(l1), _ptr(cnt), _ptr(msum), _ptr(bitmap),
                                               dyn, _OCTAV_MAX_ITERS, _stream()), "dpl_octav_run_bracket")
    out = torch.empty(plan.batch, plan.T, 3, dtype=torch.float32, device=plan.device)
    _hip.check(L.dpl_octav_finalize(_ptr(states), n_pairs, _ptr(out), _stream()), "dpl_octav_finalize")
    return out


def _octav_batch_tail(plan, tp, tensors, dynamic_sym, states_out=None, inline=False):
    """One batch of the exact-tail form on the caller's stream.  The compaction route (flat distributions, values beyond 2^14,
    a bin of 2^20 values, lists beyond their regions: rare) needs lists for the pairs that take it, which exist from the first
    batch on that asks for them — so this reads the batch's control block back (the one host synchronisation of this call;
    OctavPipeline defers it).  inline: the whole-batch lists (tp.fallback_block) are bound to the job instead, and
    dpl_octav_oneread_finish runs the route in stream order — nothing is read back."""
    L = _hip.lib()
    tab = plan.seg_table(tensors)
    state, rescue, l0, l1 = tp.single()
    k = tp.calls
    tp.calls = k + 1
    if inline and tp.fallback_block is None:
        tp.fallback_block = tp.new("fallback")
    job = tp.bind(state, rescue, l0, l1, tab, k, 1 if dynamic_sym else 0, tp.fallback_block if inline else None)
    for fn in ("dpl_octav_oneread_prepare", "dpl_octav_oneread_stream", "dpl_octav_oneread_finish"):
        _hip.check(getattr(L, fn)(C.byref(job), _stream()), fn)
    csz = C.sizeof(_hip.OctavState)
    if not inline:
        ctl = _hip.OctavState.from_buffer_copy(state[plan.n_pairs * csz:(plan.n_pairs + 1) * csz].cpu().numpy().tobytes())
        if ctl.cnt_le:
            tp.fallback = tp.compaction(job, state, torch.cuda.current_stream(plan.device), tp.fallback)
    out = torch.empty(plan.batch, plan.T, 3, dtype=torch.float32, device=plan.device)
    _hip.check(L.dpl_octav_finalize(_ptr(state), plan.n_pairs, _ptr(out), _stream()), "dpl_octav_finalize")
    if states_out is not None:      # (the caller's view of the pairs' states and the control block, as the other forms leave them)
        n = (plan.n_pairs + 1) * csz
        if states_out.numel() >= n:
            states_out[:n].copy_(state[:n])
    return out


_PIPE_SETS = max(2, int(os.environ.get("DPL_OCTAV_PIPE_SETS", "3")))   # batches the host may run ahead of the device (OctavPipeline)


_BESIDE = 0.5


def _behind(device, stream, others, cycles=1500000):
    """How far BEHIND work on `stream` does work on each of `others` run — i.e. do they share a hardware queue: 0 .. 1, the largest
    over `others`.  Asked of the device, in its own timestamps: a spin of under two milliseconds on `stream` between two timing
    events, a marker event on the other stream issued right after — a marker stamped at the spin's start ran beside it (separate
    queues: 0.01 - 0.03), one stamped at its end waited for it (one queue: 1.0).  The spin goes on the CANDIDATE and the marker on
    the other stream because `others` is usually the default stream: the other way round — the spin on the default stream of a
    process that has not used it for timing before — the marker was stamped at 0.5 - 0.6 of the spin beside it, and at 1.0 under
    rocprofv3 whatever the queues; this way round the readings are 0.01 or 1.0 with and without the profiler
    (scripts/stream_queue_probe.py).  HOST (synchronises; a few milliseconds, once per pipeline)."""
    worst = 0.0
    for o in others:
        s0, s1, m = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        with torch.cuda.stream(stream):
            s0.record(stream)
            torch.cuda._sleep(cycles)
            s1.record(stream)
        m.record(o)
        s1.synchronize()
        m.synchronize()
        spin = max(s0.elapsed_time(s1), 1e-6)
        worst = max(worst, min(1.0, max(0.0, s0.elapsed_time(m) / spin)))
    return worst


def _runs_beside(device, stream, others):
    """Does work on `stream` run beside work on each of `others` (separate hardware queues)?"""
    return _behind(device, stream, others) < _BESIDE


def _separate_stream(device, others, tries=6):
    """A normal-priority stream whose work runs beside that of `others`: the first of `tries` pool streams that does — or, should
    none be clearly beside, the one that was least behind."""
    best, best_b = None, 2.0
    for _ in range(tries):
        s = torch.cuda.Stream(device)
        b = _behind(device, s, others)
        if b < best_b:
            best, best_b = s, b
        if b < _BESIDE:
            break
    return best


class _PipeSet:
    """One of a rotation's S sets: what a batch in flight holds until the host settles it, S submits later.  Two state blocks,
    used alternately: call k's must survive until the host has read it; the next call's, k + S, is initialised behind call k."""
    __slots__ = ("S", "blocks", "rescue", "host_states", "base_host", "done", "refs", "job", "k", "pending")

    def __init__(self, tp, S):
        self.S, n = S, tp.n_pairs
        self.blocks = (tp.new("state"), tp.new("state"))
        self.rescue = tp.new("rescue")
        # (pinned: what _settle needs of a batch is on the host by the time it looks, and what it uploads leaves without a wait)
        self.host_states = torch.zeros((n + 1) * C.sizeof(_hip.OctavState), dtype=torch.uint8).pin_memory()
        self.base_host = torch.zeros(8 * (n + 1), dtype=torch.uint8).pin_memory()
        # submit fills these: the event behind the batch's side-stream work, (tensors, pointer table, rows) held until sync(),
        # the bound job, the call number (-1: not used since creation or reset), whether the batch is still to be settled
        self.done = self.refs = self.job = None
        self.k, self.pending = -1, False

    def block(self, k):
        """The state block of call k: the one place that maps a call number to a block."""
        return self.blocks[(k // self.S) % 2]


class _Rotation:
    """An OctavPipeline's scratch on one plan (every size is the C plan's, dpl_octav_plan_sizes): S sets, one list per stream
    that carries streaming kernels, one rescue list, the compaction route's arena; the call counter (call k: set k % S)."""
    __slots__ = ("plan", "tp", "S", "calls", "sets", "list0", "list1", "fallback", "__weakref__")

    def __init__(self, plan, tp, n_lanes):
        # (_PIPE_SETS is read here alone: a rotation runs on the S it was built with)
        self.plan, self.tp, self.S, self.calls = plan, tp, _PIPE_SETS, 0
        self.sets = [_PipeSet(tp, self.S) for _ in range(self.S)]
        self.list0, self.list1 = [tp.new("list") for _ in range(max(1, n_lanes))], tp.new("list")
        self.fallback = None    # _settle: the compaction route's arena, from the first batch that asks for it
        plan._octav_rotations.add(self)

    def restart(self):      # TensorSetPlan.octav_reset(), nothing in flight
        self.calls = 0
        for st in self.sets:
            st.k = -1


class OctavPipeline:
    """OCTAV over a RUN of batches in the exact-tail form on streams of its own.  Same kernels, same results as octav_batch.

        pipe = OctavPipeline(dynamic_sym)
        rows = [pipe.submit(plan, tensors) for ...]     # [B, T, 3] each, NOT valid yet
        pipe.sync()                                     # rows are valid for work on the caller's stream

    Lane streams (two, in rotation, each behind the caller's stream as of the submit): the streaming kernel, which also walks
    every pair — batch i + 1 starts while batch i drains.  Side stream, behind the streaming kernel of batch i and beside that
    of batch i + 1: the rescue of the pairs a walk could not finish (on the device, no host round trip), the result rows, the
    state and the threshold snapshot for batch i + 3.
    The pipeline OWNS its rotation per plan (_Rotation): two pipelines may run the same plan (they share only what the plan has
    learned: maxima taken into its threshold history).
    The control block of a batch (listed values, rescued pairs, pairs left for the compaction route) is copied to pinned memory
    and read when the set comes up for reuse three submits later (or in sync()): statistics, and — only when the count is
    non-zero — the compaction route for that batch.  The activations of a batch, its pointer table and its result stay
    referenced from the set until then; the host runs at most three batches ahead (DPL_OCTAV_PIPE_SETS; with two the host waited
    for side-stream work that ends with the previous streaming kernel).  A tensor set with a pair above 64 slices runs
    octav_batch (the two-read form) on the caller's stream instead."""

    def __init__(self, dynamic_sym, device=None, lanes=None):
        self._side_handle = None        # dpl_stream_create's (DPL_OCTAV_SIDE_PRIO > 0): __del__ destroys it
        self.dyn = 1 if dynamic_sym else 0
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        n_lanes = int(os.environ.get("DPL_OCTAV_LANES", "0")) or (2 if lanes is None else int(lanes))
        # The side stream: NORMAL priority, on a hardware queue of its own.  High priority (rounds 4 - 5) lets its kernels take over
        # from the streaming kernel's waves whenever the process' streams land on the queues that way (one stream 0.75 ms per batch
        # on the ResNet-50 sweep against 0.60; scripts/lanes1_after_lanes2.py, profiles/r06/ab_side_prio.txt); low priority (a stream
        # of the library's own making, dpl_stream_create) starves the rescue and with it the set the host waits for (0.77).  But a
        # normal-priority stream may SHARE its hardware queue with the caller's stream — four queues per priority class, handed out
        # in creation order — and then the rescue of batch i and the streaming kernel of batch i + 1 run one after the other (1.17 ms
        # under the profiler on one box, 0.71 on another after a two-lane pipeline had been created first): _separate_stream asks
        # the device.  DPL_OCTAV_SIDE_PRIO = -1 / 0 / 1 (high / normal / low): a fixed priority, no questions asked.
        prio = os.environ.get("DPL_OCTAV_SIDE_PRIO")
        if prio in (None, ""):
            self.side = _separate_stream(self.device, [torch.cuda.current_stream(self.device)])
        elif int(prio) > 0:
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                _hip.check(_hip.lib().dpl_stream_create(int(prio), C.byref(h)), "dpl_stream_create")
            self._side_handle = h.value
            self.side = torch.cuda.ExternalStream(h.value, self.device)
        else:
            self.side = torch.cuda.Stream(self.device, priority=int(prio))
        # The streaming kernels of consecutive batches go to two streams of the pipeline's own in rotation (each behind the
        # caller's stream as of its submit), so that batch i + 1 starts while batch i drains: the last workgroups of a batch are
        # the pairs whose walks took longest (raised thresholds, long lists) and hold a few slots while the rest of the chip idles
        # — same-box A/B (scripts/mse_run.py): images alike +- 0, +- 10 % jitter - 3.5 %, feature maps at +- 30 % - 5.5 %,
        # ViT-B/16 - 0.7 %; three streams: + 3 ... 6 % (three kernels share the slots).  lanes = 1 (or DPL_OCTAV_LANES=1): the
        # caller's stream — what a caller that runs a network forward between two submits wants (forward_net_octav: beside the
        # next forward's convolutions the streaming kernel costs the forward 10 % and the loop 6 %, scripts/e2e_lanes_ab.sh).
        self.lanes = []
        if n_lanes >= 2:       # (each on a queue of its own too: two lanes on one queue would not overlap)
            for _ in range(n_lanes):
                self.lanes.append(_separate_stream(self.device, [torch.cuda.current_stream(self.device), self.side] + self.lanes))
        self._plans = {}          # id(plan) -> _Rotation (which keeps the plan alive)
        # record_events = True: per submit a (start, end) pair of timing events around the streaming kernel ON ITS LANE, kept in
        # .events (what --timing_json reports as the statistics' GPU seconds: the caller's stream no longer carries the kernel)
        self.record_events = False
        self.events = []
        # statistics: batches settled, batches / (image, tensor) pairs whose walk was refused (rescued or compaction route)
        self.reset_stats()

    def __del__(self):
        if self._side_handle:
            try:
                self.side.synchronize()
                _hip.lib().dpl_stream_destroy(C.c_void_p(self._side_handle))
            except Exception:   # noqa: BLE001  (interpreter shutdown)
                pass

    def reset_stats(self):
        self.batches = self.fallback_batches = self.fallback_pairs = self.compaction_pairs = 0
        self.tiles_reread = self.raises = 0
        self.list_share = self.max_share = 0.0    # listed values / elements (running mean / maximum over the settled batches)

    def _rotation(self, plan, tp):
        rot = self._plans.get(id(plan))
        if rot is None:
            rot = self._plans[id(plan)] = _Rotation(plan, tp, len(self.lanes))
        return rot

    def scratch_bytes(self, plan):
        """Device bytes of this pipeline's OCTAV scratch on `plan`: tables, history, state / rescue blocks, lists, and the
        compaction route's lists if a batch has asked for them."""
        rot = self._plans.get(id(plan))
        if rot is None:
            return None
        bufs = [rot.tp.tables, rot.tp.history, rot.list1, *rot.list0] + [x for st in rot.sets for x in (*st.blocks, st.rescue)]
        return sum(x.numel() for x in bufs) + (rot.fallback.numel() if rot.fallback is not None else 0)

    def _prepare(self, rot, st, k, stream):
        """State block + threshold snapshot for this pipeline's call number k on the plan (set `st` lends its rescue block to the
        job; prepare reads no tensors: the pointer table argument is a stand-in)."""
        job = rot.tp.bind(st.block(k), st.rescue, rot.list0[0], rot.list1, rot.list1, k, self.dyn)
        _hip.check(_hip.lib().dpl_octav_oneread_prepare(C.byref(job), C.c_void_p(stream)), "dpl_octav_oneread_prepare")

    def _finish(self, rot, st):
        """Side stream: results of the set's batch -> its output rows, the set made ready for its next use, completion event."""
        side = self.side.cuda_stream
        _hip.check(_hip.lib().dpl_octav_finalize(_ptr(st.block(st.k)), rot.plan.n_pairs, _ptr(st.refs[2]), side), "dpl_octav_finalize")
        self._prepare(rot, st, st.k + rot.S, side)    # off the caller's stream: the set's next use is S calls away
        st.done = self.side.record_event()

    def _settle(self, rot, st):
        """HOST: read the statistics the set's last batch left in pinned memory (the walk finished long ago: the set comes up
        for reuse S submits later).  Nothing is launched here unless pairs are left for the compaction route: the pairs a walk
        could not finish are rescued on the device, without the host (submit)."""
        if not st.pending:
            return
        st.pending = False
        st.done.synchronize()
        plan = rot.plan
        ctl = _hip.OctavState.from_buffer_copy(st.host_states.numpy(), plan.n_pairs * C.sizeof(_hip.OctavState))    # the control block
        # listed values; pairs rescued by a re-read of the pair + pairs that ended on the compaction route
        listed, failed = float(ctl.sum), int(ctl.len0) + int(ctl.cnt_le)
        self.compaction_pairs += int(ctl.cnt_le)
        self.raises += int(ctl.iters)              # thresholds raised on the fly (waves that listed beyond their budget)
        self.tiles_reread += int(ctl.reserved)     # 1024-element tiles holding a non-zero value outside the window
        self.batches += 1
        share = listed / max(1, plan.batch * sum(plan.elems))
        self.list_share = share if self.batches == 1 else 0.9 * self.list_share + 0.1 * share
        self.max_share = max(self.max_share, share)
        if failed:
            self.fallback_pairs += failed
            self.fallback_batches += 1
        if ctl.cnt_le:
            # what neither the walk nor the rescue could finish (a bracket that cannot be formed: flat distributions, values
            # beyond 2^14, a list beyond its region): the compaction route, launched only now that the count is known — the set's
            # batch is S submits old, its tensors are still referenced — on lists with regions for just the pairs that need them
            # (laid out from the states in pinned memory), its results written over the batch's output rows
            rot.fallback = rot.tp.compaction(st.job, st.block(st.k), self.side, rot.fallback, st.host_states, st.base_host)
            self._finish(rot, st)

    def submit(self, plan, tensors):
        form = _default_form()
        tp = plan.octav_tail() if form == "tail" else None
        if tp is None:      # another form was asked for, or a pair above 64 slices: one batch at a time on the caller's stream
            return octav_batch(plan, tensors, bool(self.dyn), form="bracket" if form == "tail" else form)
        main = caller = torch.cuda.current_stream(plan.device)
        rot = self._rotation(plan, tp)
        k = rot.calls
        if self.lanes:
            main = self.lanes[k % len(self.lanes)]
        cur = rot.sets[k % rot.S]
        self._settle(rot, cur)
        if cur.done is not None:
            main.wait_event(cur.done)           # everything that last used this set has finished
        tab = plan.seg_table(tensors)
        out = torch.empty(plan.batch, plan.T, 3, dtype=torch.float32, device=plan.device)
        rot.calls = k + 1                       # (only now: a tensor set that seg_table refuses takes no call number)
        if main is not caller:
            main.wait_stream(caller)            # the batch's activations and its pointer table are the caller's stream's work
        cur.refs = (tensors if isinstance(tensors, BoundSet) else list(tensors), tab, out)
        L = _hip.lib()
        if cur.k < 0:       # (a set used before finds its block prepared: its last call, k - S, ended on _finish)
            self._prepare(rot, cur, k, main.cuda_stream)
        cur.k = k
        state = cur.block(k)
        job = cur.job = tp.bind(state, cur.rescue, rot.list0[k % len(rot.list0)], rot.list1, tab, k, self.dyn)
        if self.record_events:
            began = torch.cuda.Event(enable_timing=True)
            began.record(main)
        _hip.check(L.dpl_octav_oneread_stream(C.byref(job), C.c_void_p(main.cuda_stream)), "dpl_octav_oneread_stream")
        streamed = torch.cuda.Event(enable_timing=self.record_events)
        streamed.record(main)
        if self.record_events:
            self.events.append((began, streamed))
        self.side.wait_event(streamed)
        # the rescue of the pairs a walk could not finish, on the device: no host round trip decides anything
        _hip.check(L.dpl_octav_oneread_finish(C.byref(job), C.c_void_p(self.side.cuda_stream)), "dpl_octav_oneread_finish")
        with torch.cuda.stream(self.side):
            # the pairs' states and the control block behind them — statistics, and whether the compaction route is needed, which
            # lays its lists out from the states (_settle): 80 bytes per pair behind every batch instead of a read-back
            cur.host_states.copy_(state[:cur.host_states.numel()], non_blocking=True)
        self._finish(rot, cur)
        cur.pending = True
        return out

    def sync(self):
        """Settle every outstanding batch (host waits for the walks), order the caller's stream after the side stream and
        let go of the batches' tensors."""
        for rot in self._plans.values():
            for st in sorted(rot.sets, key=lambda q: q.k):
                self._settle(rot, st)
        for stream in [self.side] + self.lanes:
            torch.cuda.current_stream(self.device).wait_stream(stream)
        for rot in self._plans.values():
            for st in rot.sets:
                st.refs = None


# ------------------------------------------------------------------------------- single-tensor conveniences
def minmax(x):
    """(min, max) of one device tensor as a fp32 device tensor [2] (NaN if x holds a NaN)."""
    _require_cuda(x)
    plan = TensorSetPlan([x.numel()], 1, x.device)
    acc = CalibAccumulators(1, x.device)
    acc.minmax_accumulate(plan, [x])
    lo, hi = acc.finalize_minmax()
    return torch.stack([lo[0], hi[0]])


def abs_hist(x, bins, gmin, gmax):
    """np.histogram(|x|, bins, (0, max(gmax, -gmin)))[0] as an int64 device tensor [bins]."""
    _require_cuda(x)
    plan = TensorSetPlan([x.numel()], 1, x.device)
    acc = CalibAccumulators(1, x.device, bins)
    acc.set_minmax(torch.tensor([gmin], dtype=torch.float32, device=x.device),
                   torch.tensor([gmax], dtype=torch.float32, device=x.device))
    acc.hist_prepare()
    acc.abs_hist_accumulate(plan, [x])
    return acc.hist[0], acc


def rowwise_minmax(w2d, out=None):
    """Per-row (min, max) of a [rows, cols] fp32 device matrix (basic_algorithm.py:88-90); out = (lo, hi): where to write them."""
    _require_cuda(w2d, "w2d")
    rows, cols = w2d.shape
    if out is None:
        lo = torch.empty(rows, dtype=torch.float32, device=w2d.device)
        hi = torch.empty(rows, dtype=torch.float32, device=w2d.device)
    else:       # (a graph's initializers: slices of one result buffer, read back in one transfer)
        lo, hi = out
        _require_cuda(lo, "out[0]")
        _require_cuda(hi, "out[1]")
        if lo.numel() != rows or hi.numel() != rows:
            raise _hip.DipoorletHipError(f"rowwise_minmax: out holds {lo.numel()} / {hi.numel()} values for {rows} rows")
    _hip.check(_hip.lib().dpl_rowwise_minmax(_ptr(w2d), rows, cols, _ptr(lo), _ptr(hi), _stream()),
               "dpl_rowwise_minmax")
    return lo, hi


def colwise_absmax(x, acc=None):
    """Running per-channel max |x| of a channels-last fp32 device tensor (dpl_colwise_absmax; the statistic of --smooth): x of any
    rank >= 1, contiguous (never copied here), seen as [-1, C] with C = x.shape[-1]; acc <- np.maximum(acc, np.abs(x).max(0)), bit for
    bit (a NaN in a column or already in acc stays NaN).  acc: fp32 [C] on x's device holding non-negative values, zeroed by its
    owner before the first batch; None: a zeroed one is made.  Runs on the current stream, no host synchronisation.  Returns acc."""
    _require_cuda(x, "x")
    if x.dim() < 1:
        raise _hip.DipoorletHipError("colwise_absmax: x must have at least one axis")
    cols = int(x.shape[-1])
    rows = x.numel() // cols if cols else 0
    if acc is None:
        acc = torch.zeros(cols, dtype=torch.float32, device=x.device)
    else:
        _require_cuda(acc, "acc")
        if acc.numel() != cols or acc.device != x.device:
            raise _hip.DipoorletHipError(f"colwise_absmax: acc holds {acc.numel()} values for {cols} channels")
    _hip.check(_hip.lib().dpl_colwise_absmax(_ptr(x), rows, cols, _ptr(acc), _stream()), "dpl_colwise_absmax")
    return acc


FQ_PRE = {None: 0, "none": 0, "relu": 1, "add_relu": 2}     # include/dipoorlet_hip.h DPL_FQ_PRE_*


def _fq_args(x, scale, axis, pre, x2, zero_point=None):
    """The argument checks the Q/DQ kernels of both number formats share -> (pre code, scale and zero point as the kernel takes
    them, channels, inner); zero_point: the integer grid's only."""
    _require_cuda(x, "x")
    code = FQ_PRE[pre]
    if code == 2:
        _require_cuda(x2, "x2")
        if x2.shape != x.shape or x2.dtype != torch.float32 or not x2.is_contiguous():
            raise _hip.DipoorletHipError("fake_quant(pre='add_relu'): x2 must be a contiguous fp32 tensor of x's shape")
    # (a graph walk issues one of these per tensor: no conversion calls when the parameters already are what the kernel takes)
    if not (scale.device == x.device and scale.dtype == torch.float32 and scale.dim() == 1 and scale.is_contiguous()):
        scale = scale.to(device=x.device, dtype=torch.float32).contiguous().reshape(-1)
    nch = scale.numel()
    if zero_point is not None:
        if not (zero_point.device == x.device and zero_point.dtype == torch.int32 and zero_point.dim() == 1 and zero_point.is_contiguous()):
            zero_point = zero_point.to(device=x.device, dtype=torch.int32).contiguous().reshape(-1)
        if zero_point.numel() != nch:
            raise _hip.DipoorletHipError("scale and zero_point lengths differ")
    inner = 1
    if nch > 1:
        if axis is None:
            raise _hip.DipoorletHipError("per-channel fake_quant needs an axis")
        # (a negative axis counts from the end, as ONNX QuantizeLinear's does: x.shape[axis + 1:] with axis = -1 would be x.shape[0:])
        if not isinstance(axis, int) or not -x.dim() <= axis < x.dim():
            raise _hip.DipoorletHipError(f"fake_quant: axis {axis!r} out of range for a tensor of {x.dim()} dimension(s)")
        axis %= x.dim()
        if x.shape[axis] != nch:
            raise _hip.DipoorletHipError(f"axis {axis} has {x.shape[axis]} channels, scale has {nch}")
        for d in x.shape[axis + 1:]:
            inner *= int(d)
    return code, scale, zero_point, nch, inner


def _fq_out(who, x, out):
    """Where the Q/DQ kernels write: a new tensor, or the caller's `out` (x itself is allowed) — which the kernel fills with
    x.numel() fp32 values in x's order, so anything but a contiguous fp32 tensor of x's shape on x's device is refused."""
    if out is None:
        return torch.empty_like(x)
    if not (isinstance(out, torch.Tensor) and out.device == x.device and out.dtype == torch.float32 and out.shape == x.shape
            and out.is_contiguous()):
        raise _hip.DipoorletHipError(f"{who}: out must be a contiguous float32 tensor of x's shape {list(x.shape)} on x's device")
    return out


def fake_quant(x, scale, zero_point, qlo, qhi, axis=None, out=None, pre=None, x2=None):
    """Fused QuantizeLinear -> DequantizeLinear (quantize.py:197-239) on the device.

    scale: fp32 device tensor [1] or [C]; zero_point: int32 device tensor of the same length;
    axis: channel axis when len(scale) > 1 (negative: from the end).  y = (clamp(rint(x/scale)+zp, qlo, qhi) - zp) * scale.
    out: where to write — a contiguous fp32 tensor of x's shape on x's device (x itself: in place); None: a new tensor.
    pre: the producer's activation applied on the way in (dpl_fake_quant_pre) — 'relu': fq(max(x, 0)); 'add_relu':
    fq(max(x + x2, 0)), x2 of x's shape (the residual Add of a bottleneck and its ReLU) — for a forward that does not expose the
    producer's output (the merge-ReLU rule, quantize.py:50-55, puts the Q/DQ pair directly behind that ReLU).
    """
    code, scale, zero_point, nch, inner = _fq_args(x, scale, axis, pre, x2, zero_point)
    y = _fq_out("fake_quant", x, out)
    _hip.check(_hip.lib().dpl_fake_quant_pre(code, _ptr(x), _ptr(x2) if code == 2 else None, _ptr(y), x.numel(), _ptr(scale),
                                             _ptr(zero_point), nch, inner, int(qlo), int(qhi), _stream()), "dpl_fake_quant_pre")
    return y


def fake_quant_fp8(x, scale, axis=None, out=None, pre=None, x2=None):
    """The same pair on the OCP FP8 E4M3 grid (dpl_fake_quant_fp8; quantisation type 'Float8E4M3FN'): y = fl32(e4m3_round(fl32(x /
    scale)) * scale), the nearest e4m3fn value, ties to even, saturating at +-448, NaN kept (tests/fp8_model.py is the definition).
    scale: fp32 device tensor [1] or [C]; axis, out, pre, x2: as fake_quant.  No zero point, no integer bounds."""
    code, scale, _, nch, inner = _fq_args(x, scale, axis, pre, x2)
    y = _fq_out("fake_quant_fp8", x, out)
    _hip.check(_hip.lib().dpl_fake_quant_fp8(code, _ptr(x), _ptr(x2) if code == 2 else None, _ptr(y), x.numel(), _ptr(scale),
                                             nch, inner, _stream()), "dpl_fake_quant_fp8")
    return y


MX_ELEM = {"mxfp8": _hip.MX_E4M3, "mxfp4": _hip.MX_E2M1,     # include/dipoorlet_hip.h DPL_MX_*
           "mxfp6_e2m3": _hip.MX_E2M3, "mxfp6_e3m2": _hip.MX_E3M2}
MX_CODE_BITS = {"mxfp8": 8, "mxfp4": 4, "mxfp6_e2m3": 6, "mxfp6_e3m2": 6}     # of an element code in the packed form (mx_encode)
MX_ELEM_MIXED = ("mxfp8", "mxfp4")      # what mx_gemm_err (--mx_mixed) and gptq_mx_block (--mx_gptq) are held to: no FP6 format
MX_BLOCK = 32
_MX_ELEM_WORDS = "elem must be 'mxfp8' or 'mxfp4' (or 'mxfp6_e2m3' / 'mxfp6_e3m2')"


def fake_quant_mx(x, axis, elem, out=None, scales=None):
    """The OCP Microscaling Q/DQ pair (dpl_fake_quant_mx; tests/mx_model.py is the definition): every 32 consecutive elements
    along `axis` (negative: from the end) share a power-of-two scale taken from their largest |v|, and are rounded to FP8 E4M3
    (elem 'mxfp8'), FP6 E2M3 / E3M2 ('mxfp6_e2m3' / 'mxfp6_e3m2'; tests/mx_fp6_model.py is their definition) or FP4 E2M1 ('mxfp4') under it.  No parameters: the scales are the data's own.  out: as fake_quant (may be x);
    scales: an optional uint8 device tensor of [outer, ceil(K / 32), inner] elements that receives the E8M0 codes (0xFF: a block
    that holds a NaN or an infinity, whose elements all come out NaN)."""
    _require_cuda(x, "x")
    axis, outer, k, inner = _mx_split("fake_quant_mx", tuple(x.shape), axis, elem)
    y = _mx_out("fake_quant_mx", out, x.shape, x.device, "x's shape and device")
    if scales is not None:
        want = outer * (-(-k // MX_BLOCK)) * inner
        if not (isinstance(scales, torch.Tensor) and scales.is_cuda and scales.device == x.device and scales.dtype == torch.uint8
                and scales.is_contiguous() and scales.numel() == want):
            raise _hip.DipoorletHipError(f"fake_quant_mx: scales must be a contiguous uint8 device tensor of {want} elements "
                                         f"([outer, ceil(K / {MX_BLOCK}), inner] = [{outer}, {-(-k // MX_BLOCK)}, {inner}])")
    _hip.check(_hip.lib().dpl_fake_quant_mx(MX_ELEM[elem], _ptr(x), _ptr(y), outer, k, inner, None if scales is None else _ptr(scales),
                                            _stream()), "dpl_fake_quant_mx")
    return y


def _mx_out(who, out, shape, device, what):
    """Where an MX op writes its fp32 result: the caller's `out`, which must have `shape` on `device` (`what`: the message's words
    for the two), or a new tensor."""
    if out is None:
        return torch.empty(tuple(shape), dtype=torch.float32, device=device)
    _require_cuda(out, "out")
    if tuple(out.shape) != tuple(shape) or out.device != device:
        raise _hip.DipoorletHipError(f"{who}: out must have {what}")
    return out


def _mx_split(who, shape, axis, elem):
    """The argument checks fake_quant_mx, mx_encode and mx_decode share -> (axis from the front, outer, k, inner)."""
    if elem not in MX_ELEM:
        raise _hip.DipoorletHipError(f"{who}: {_MX_ELEM_WORDS}, got {elem!r}")
    nd = len(shape)
    if not isinstance(axis, int) or not -nd <= axis < nd:
        raise _hip.DipoorletHipError(f"{who}: axis {axis!r} out of range for a tensor of {nd} dimension(s)")
    axis %= nd
    outer = inner = 1
    for d in shape[:axis]:
        outer *= int(d)
    for d in shape[axis + 1:]:
        inner *= int(d)
    return axis, outer, int(shape[axis]), inner


def mx_packed_shapes(shape, axis, elem):
    """(codes shape, scales shape) of an MX tensor of `shape` blocked along `axis` as mx_encode writes it: K-innermost, [*outer
    dims, *inner dims, Kp (mxfp8), Kp * 3 / 4 (the two mxfp6) or Kp / 2 (mxfp4)] and [..., Kp / 32] with Kp = 32 * ceil(K / 32)."""
    axis, _, k, _ = _mx_split("mx_packed_shapes", tuple(shape), axis, elem)
    kp = MX_BLOCK * -(-k // MX_BLOCK)
    lead = tuple(int(d) for d in shape[:axis]) + tuple(int(d) for d in shape[axis + 1:])
    return lead + (kp * MX_CODE_BITS[elem] // 8,), lead + (kp // MX_BLOCK,)


def mx_encode(x, axis, elem):
    """`--mx_pack`: what fake_quant_mx(x, axis, elem) computes, as bytes (dpl_mx_encode; tests/mx_pack_model.py is the definition)
    -> (codes, scales), uint8 device tensors.  scales: the E8M0 byte per block (0xFF: the block holds a NaN or an infinity);
    codes: OCP FP8 E4M3FN bytes ('mxfp8'; 0x7F in a 0xFF block), E2M1 nibbles, two to a byte, the even index along `axis` in the
    low nibble ('mxfp4'; 0 in a 0xFF block), or 6-bit codes, a block's 32 as one little-endian string of 192 bits with code i in
    bits [6 i, 6 i + 6) (the two 'mxfp6'; 0 in a 0xFF block).  Both are K-INNERMOST — mx_packed_shapes(x.shape, axis, elem): the block axis moves
    to the end, padded with code 0 to a multiple of 32 —, which for an axis that is not the last is a transpose of x's element
    order, and not the order of fake_quant_mx's scales=."""
    _require_cuda(x, "x")
    _, outer, k, inner = _mx_split("mx_encode", tuple(x.shape), axis, elem)
    cs, ss = mx_packed_shapes(x.shape, axis, elem)
    codes = torch.empty(cs, dtype=torch.uint8, device=x.device)
    scales = torch.empty(ss, dtype=torch.uint8, device=x.device)
    _hip.check(_hip.lib().dpl_mx_encode(MX_ELEM[elem], _ptr(x), outer, k, inner, _ptr(codes), _ptr(scales), _stream()), "dpl_mx_encode")
    return codes, scales


def _mx_block_shape(shape, axis):
    """`shape` with the block axis (counted from the front) replaced by its number of blocks: the shape of one byte per block."""
    return tuple(int(d) for d in shape[:axis]) + (-(-int(shape[axis]) // MX_BLOCK),) + tuple(int(d) for d in shape[axis + 1:])


def _mx_given_scales(who, x, axis, scales):
    """The check of the `scales` fake_quant_mx_scaled and mx_encode_scaled read: one byte per block, in x's own order."""
    want = _mx_block_shape(x.shape, axis)
    if not (isinstance(scales, torch.Tensor) and scales.is_cuda and scales.device == x.device and scales.dtype == torch.uint8
            and scales.is_contiguous() and scales.numel() == int(np.prod(want, dtype=np.int64))):
        raise _hip.DipoorletHipError(f"{who}: scales must be a contiguous uint8 device tensor of shape {list(want)} (x's, with the block "
                                     f"axis replaced by ceil(K / {MX_BLOCK})) on x's device")


def mx_scale_search(x, axis, elem, err=None):
    """`--mx_scale_search` (dpl_mx_scale_search; tests/mx_scale_model.py is the definition): per block of 32 along `axis`, whichever
    of the floor-rule shared exponent se0 (fake_quant_mx's) and se0 + 1 gives the smaller squared Q/DQ error — se0 + 1 only where it
    is strictly smaller, and never above 127 - emax.  -> a uint8 device tensor shaped like x with the block axis replaced by
    ceil(K / 32): the E8M0 bytes (0xFF: the block holds a NaN or an infinity), in the order of fake_quant_mx's scales=.
    err: an optional contiguous fp64 device tensor of that shape + (2,) that receives, per block, the error at the floor and the
    error at the chosen byte (+inf for a 0xFF block) — fp64 sums of exact squares in a fixed order."""
    _require_cuda(x, "x")
    axis, outer, k, inner = _mx_split("mx_scale_search", tuple(x.shape), axis, elem)
    shape = _mx_block_shape(x.shape, axis)
    if err is not None:
        if not (isinstance(err, torch.Tensor) and err.is_cuda and err.device == x.device and err.dtype == torch.float64
                and err.is_contiguous() and err.numel() == 2 * int(np.prod(shape, dtype=np.int64))):
            raise _hip.DipoorletHipError(f"mx_scale_search: err must be a contiguous float64 device tensor of shape {list(shape) + [2]} on x's device")
    scales = torch.empty(shape, dtype=torch.uint8, device=x.device)
    _hip.check(_hip.lib().dpl_mx_scale_search(MX_ELEM[elem], _ptr(x), outer, k, inner, _ptr(scales), None if err is None else _ptr(err),
                                              _stream()), "dpl_mx_scale_search")
    return scales


def fake_quant_mx_scaled(x, axis, elem, scales, out=None):
    """fake_quant_mx under GIVEN E8M0 bytes (dpl_fake_quant_mx_scaled; tests/mx_scale_model.py is the definition): scales is what
    mx_scale_search returns (any bytes are defined: 0xFF, a byte above 254 - emax, or a NaN or an infinity in the block make every
    element of the block NaN).  With the bytes fake_quant_mx writes it equals fake_quant_mx bit for bit.  out: as fake_quant_mx."""
    _require_cuda(x, "x")
    axis, outer, k, inner = _mx_split("fake_quant_mx_scaled", tuple(x.shape), axis, elem)
    _mx_given_scales("fake_quant_mx_scaled", x, axis, scales)
    y = _mx_out("fake_quant_mx_scaled", out, x.shape, x.device, "x's shape and device")
    _hip.check(_hip.lib().dpl_fake_quant_mx_scaled(MX_ELEM[elem], _ptr(x), _ptr(y), outer, k, inner, _ptr(scales), _stream()),
               "dpl_fake_quant_mx_scaled")
    return y


def mx_encode_scaled(x, axis, elem, scales):
    """mx_encode under GIVEN E8M0 bytes (dpl_mx_encode_scaled; tests/mx_scale_model.py is the definition) -> (codes, packed scales)
    as mx_encode returns them, K-innermost.  scales: one byte per block in x's own order, what mx_scale_search returns; the packed
    scales are those bytes transposed, 0xFF where the block is a 0xFF block.  mx_decode of the result equals
    fake_quant_mx_scaled(x, axis, elem, scales) bit for bit."""
    _require_cuda(x, "x")
    axis, outer, k, inner = _mx_split("mx_encode_scaled", tuple(x.shape), axis, elem)
    _mx_given_scales("mx_encode_scaled", x, axis, scales)
    cs, ss = mx_packed_shapes(x.shape, axis, elem)
    codes = torch.empty(cs, dtype=torch.uint8, device=x.device)
    packed = torch.empty(ss, dtype=torch.uint8, device=x.device)
    _hip.check(_hip.lib().dpl_mx_encode_scaled(MX_ELEM[elem], _ptr(x), outer, k, inner, _ptr(scales), _ptr(codes), _ptr(packed), _stream()),
               "dpl_mx_encode_scaled")
    return codes, packed


def mx_decode(codes, scales, elem, shape, axis, out=None):
    """The inverse of mx_encode (dpl_mx_decode): codes / scales as mx_packed_shapes(shape, axis, elem) lays them out -> the fp32
    tensor of `shape`; mx_decode(*mx_encode(x, axis, elem), elem, x.shape, axis) equals fake_quant_mx(x, axis, elem) bit for bit.
    Defined on every byte pair: scale 0xFF and the E4M3 codes 0x7F / 0xFF give NaN, a product above fp32's range +-inf.  out: an
    optional contiguous fp32 device tensor of `shape`."""
    for t, name in ((codes, "codes"), (scales, "scales")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise _hip.DipoorletHipError(f"mx_decode: {name} must be a contiguous uint8 ROCm device tensor; dipoorlet_amd has no CPU path")
    shape = tuple(int(d) for d in shape)
    _, outer, k, inner = _mx_split("mx_decode", shape, axis, elem)
    cs, ss = mx_packed_shapes(shape, axis, elem)
    if codes.numel() != int(np.prod(cs, dtype=np.int64)) or scales.numel() != int(np.prod(ss, dtype=np.int64)) or scales.device != codes.device:
        raise _hip.DipoorletHipError(f"mx_decode: a tensor of shape {list(shape)} along axis {axis} has codes {list(cs)} and scales {list(ss)} "
                                     f"(K-innermost), got {list(codes.shape)} and {list(scales.shape)}")
    y = _mx_out("mx_decode", out, shape, codes.device, "the given shape and the codes' device")
    _hip.check(_hip.lib().dpl_mx_decode(MX_ELEM[elem], _ptr(codes), _ptr(scales), outer, k, inner, _ptr(y), _stream()), "dpl_mx_decode")
    return y


def _mx_packed_pair(who, a, b, elem_a, elem_b, dims_ok, kp, how):
    """The checks mx_gemm and mx_conv share on their two packed MX operands (codes, scales, the message's words for the leading
    dimensions), each what mx_encode writes, K-innermost -> (elem_b, A's (leading dimensions, K-blocks), B's).  dims_ok: the rule on the
    number of dimensions; kp, how: the message's name of the padded block axis and of the axis that was encoded."""
    elem_b = elem_a if elem_b is None else elem_b
    for e in (elem_a, elem_b):
        if e not in MX_ELEM:
            raise _hip.DipoorletHipError(f"{who}: {_MX_ELEM_WORDS}, got {e!r}")
    for t, name in ((a[0], "a_codes"), (a[1], "a_scales"), (b[0], "b_codes"), (b[1], "b_scales")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == a[0].device):
            raise _hip.DipoorletHipError(f"{who}: {name} must be a contiguous uint8 ROCm device tensor on one device; dipoorlet_amd has no CPU path")

    def split(codes, scales, dims, elem, label):
        bits = MX_CODE_BITS[elem]
        part = {8: "", 6: " * 3 / 4", 4: " / 2"}[bits]          # of Kp: the bytes of a row of codes
        if not (dims_ok(codes.dim()) and scales.dim() == codes.dim() and tuple(scales.shape[:-1]) == tuple(codes.shape[:-1])
                and int(codes.shape[-1]) * 8 == bits * MX_BLOCK * int(scales.shape[-1])):
            raise _hip.DipoorletHipError(f"{who}: {label} must be codes [{dims}, {kp}{part}] and scales [{dims}, {kp} / "
                                         f"{MX_BLOCK}] as mx_encode writes {elem}{how} (K-innermost), got {list(codes.shape)} and "
                                         f"{list(scales.shape)}")
        return tuple(int(d) for d in codes.shape[:-1]), int(scales.shape[-1])
    return elem_b, split(*a, elem_a, "A"), split(*b, elem_b, "B")


MX_GEMM_TILE = 64                       # rows and columns of C per workgroup of k_mx_gemm / k_mx_gemm_err (mx_plan.hpp kMxGemmTile)


def _mx_gemm_pair(who, a_codes, a_scales, b_codes, b_scales, elem_a, elem_b):
    """The operand checks of mx_gemm and mx_gemm_err -> (elem_b, A's leading dimensions, m, n, K-blocks, batch, b_batched)."""
    elem_b, ((*lead, m), nblk), ((*lead_b, n), nblk_b) = _mx_packed_pair(
        who, (a_codes, a_scales, "..., rows"), (b_codes, b_scales, "..., rows"), elem_a, elem_b, lambda nd: nd >= 2, "Kp", "")
    lead, lead_b = tuple(lead), tuple(lead_b)
    if nblk_b != nblk or lead_b not in ((), lead):
        raise _hip.DipoorletHipError(f"{who}: A is {list(lead)} x [{m}, {nblk} blocks] and B {list(lead_b)} x [{n}, {nblk_b} blocks]: the two must "
                                     "have the same number of K-blocks, and B the leading dimensions of A or none")
    batch = 1
    for d in lead:
        batch *= d
    return elem_b, lead, m, n, nblk, batch, int(lead_b == lead and lead != ())


def mx_gemm(a_codes, a_scales, b_codes, b_scales, elem_a, elem_b=None, out=None):
    """`--mx_verify`: the product of two packed MX operands on CDNA4's block-scaled matrix instruction (dpl_mx_gemm;
    tests/mx_gemm_model.py is the definition).  Both operands are what mx_encode writes, K-innermost: a_codes [*batch, m, Kp or
    Kp / 2] with a_scales [*batch, m, Kp / 32]; b_codes [*batch, n, ...] / b_scales [*batch, n, Kp / 32] with the same leading
    dimensions, or [n, ...] / [n, Kp / 32], which every batch shares.  -> fp32 [*batch, m, n], C[.., i, j] = sum over the Kp codes
    of a[.., i, :] * b[.., j, :] (pad codes included).  elem_b: B's element format when it is not A's.  A row that holds a 0xFF
    scale byte or an E4M3 NaN code makes its row (column) of C NaN.  out: an optional contiguous fp32 device tensor of that shape."""
    elem_b, lead, m, n, nblk, batch, b_batched = _mx_gemm_pair("mx_gemm", a_codes, a_scales, b_codes, b_scales, elem_a, elem_b)
    shape = lead + (m, n)
    c = _mx_out("mx_gemm", out, shape, a_codes.device, f"shape {list(shape)} and the codes' device")
    _hip.check(_hip.lib().dpl_mx_gemm(MX_ELEM[elem_a], MX_ELEM[elem_b], _ptr(a_codes), _ptr(a_scales), _ptr(b_codes), _ptr(b_scales), batch, m, n,
                                      MX_BLOCK * nblk, b_batched, _ptr(c), _stream()), "dpl_mx_gemm")
    return c


def mx_gemm_err(a_codes, a_scales, b_codes, b_scales, ref, elem_a, elem_b=None, bias=None, out=None):
    """`--mx_mixed`: mx_gemm's product held against a reference without being written (dpl_mx_gemm_err; tests/mx_mixed_model.py
    gemm_err_partials is the definition).  The operands are mx_gemm's; ref: fp32 [*batch, m, n]; bias: None or fp32 [n].  -> fp64
    [*batch, tiles_m, tiles_n, 2], per 64 x 64 tile of C the sums of d * d and of ref * ref over the tile's elements, d = (C + bias)
    - ref in fp32, each square exact in fp64 and the additions in the kernel's fixed order.  A NaN of C (mx_gemm's rule) makes its
    tile's first sum NaN.  out: an optional contiguous fp64 device tensor of that shape."""
    for e in (elem_a, elem_a if elem_b is None else elem_b):
        if e not in MX_ELEM_MIXED:
            raise _hip.DipoorletHipError(f"mx_gemm_err: elem must be 'mxfp8' or 'mxfp4' (--mx_mixed chooses between these two), got {e!r}")
    elem_b, lead, m, n, nblk, batch, b_batched = _mx_gemm_pair("mx_gemm_err", a_codes, a_scales, b_codes, b_scales, elem_a, elem_b)
    _require_cuda(ref, "ref")
    if tuple(ref.shape) != lead + (m, n) or ref.device != a_codes.device:
        raise _hip.DipoorletHipError(f"mx_gemm_err: ref must have shape {list(lead + (m, n))} and the codes' device")
    if bias is not None:
        _require_cuda(bias, "bias")
        if tuple(bias.shape) != (n,) or bias.device != a_codes.device:
            raise _hip.DipoorletHipError(f"mx_gemm_err: bias must have shape [{n}] and the codes' device")
    shape = lead + (-(-m // MX_GEMM_TILE), -(-n // MX_GEMM_TILE), 2)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=a_codes.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
              and tuple(out.shape) == shape and out.device == a_codes.device):
        raise _hip.DipoorletHipError(f"mx_gemm_err: out must be a contiguous float64 tensor of shape {list(shape)} on the codes' device")
    _hip.check(_hip.lib().dpl_mx_gemm_err(MX_ELEM[elem_a], MX_ELEM[elem_b], _ptr(a_codes), _ptr(a_scales), _ptr(b_codes), _ptr(b_scales), batch, m,
                                          n, MX_BLOCK * nblk, b_batched, _ptr(ref), None if bias is None else _ptr(bias), _ptr(out), _stream()),
               "dpl_mx_gemm_err")
    return out


def mx_conv(a_codes, a_scales, b_codes, b_scales, elem_a, elem_b=None, *, strides, pads, dilations, out_hw, out=None):
    """`--mx_conv`: a convolution (group 1) of two packed MX operands on the block-scaled matrix instruction, as an implicit GEMM
    (dpl_mx_conv; tests/mx_conv_model.py is the definition).  Both operands are what mx_encode writes along axis 1: a_codes [n, h, w,
    Cp or Cp / 2] with a_scales [n, h, w, Cp / 32] of an [n, c, h, w] activation, b_codes [cout, kh, kw, ...] / b_scales [cout, kh, kw,
    Cp / 32] of a [cout, c, kh, kw] weight.  strides (sh, sw), pads (top, left), dilations (dh, dw), out_hw (oh, ow): the caller's —
    nothing is derived here; a tap outside the image contributes nothing.  -> fp32 [n, oh, ow, cout] (NHWC).  elem_b: B's element
    format when it is not A's.  An output is NaN if a block inside one of its in-image taps, or any block of its weight row, holds a
    0xFF scale byte or an E4M3 NaN code.  out: an optional contiguous fp32 device tensor of that shape."""
    elem_b, ((n, h, w), cb), ((cout, kh, kw), cb_b) = _mx_packed_pair(
        "mx_conv", (a_codes, a_scales, "n, h, w"), (b_codes, b_scales, "cout, kh, kw"), elem_a, elem_b, lambda nd: nd == 4, "Cp", " along axis 1")
    if cb_b != cb:
        raise _hip.DipoorletHipError(f"mx_conv: A has {cb} channel block(s) a pixel and B {cb_b}: the two must have the same number of K-blocks a tap")
    geom = []
    for v, name in ((strides, "strides"), (pads, "pads"), (dilations, "dilations"), (out_hw, "out_hw")):
        if not (isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(d, (int, np.integer)) and not isinstance(d, bool) for d in v)):
            raise _hip.DipoorletHipError(f"mx_conv: {name} must be two integers, got {v!r}")
        geom.append((int(v[0]), int(v[1])))
    (sh, sw), (pt, pl), (dh, dw), (oh, ow) = geom
    if oh < 0 or ow < 0:
        raise _hip.DipoorletHipError(f"mx_conv: out_hw must not be negative, got {out_hw!r}")
    shape = (n, oh, ow, cout)
    c = _mx_out("mx_conv", out, shape, a_codes.device, f"shape {list(shape)} and the codes' device")
    _hip.check(_hip.lib().dpl_mx_conv(MX_ELEM[elem_a], MX_ELEM[elem_b], _ptr(a_codes), _ptr(a_scales), _ptr(b_codes), _ptr(b_scales), n, h, w,
                                      MX_BLOCK * cb, cout, kh, kw, sh, sw, pt, pl, dh, dw, oh, ow, _ptr(c), _stream()), "dpl_mx_conv")
    return c


def mx_matmul(x, w_codes, w_scales, elem, elem_w=None):
    """x . W on the block-scaled matrix instruction: x (fp32 [..., m, K]) is encoded along its last axis as `elem` (mx_encode), W is
    already packed — mx_encode(w, -2, elem_w) of a [K, N] weight, i.e. [N, Kp] codes — and the two go through mx_gemm -> [..., m, N]."""
    if not isinstance(x, torch.Tensor) or x.dim() < 2:
        raise _hip.DipoorletHipError("mx_matmul: x must be a tensor of at least two dimensions, [..., m, K]")
    a_codes, a_scales = mx_encode(x, -1, elem)
    return mx_gemm(a_codes, a_scales, w_codes, w_scales, elem, elem if elem_w is None else elem_w)


def hadamard32(x, out=None):
    """The block-Hadamard rotation of `--mx_rotate` (dpl_hadamard32; tests/mx_rotate_model.py fwht32 is the definition): every 32
    consecutive elements along the last axis are multiplied by the symmetric +-1 Sylvester matrix H32 (no normalisation: the
    constant operand of the product carries the 2^-5).  x: a contiguous fp32 device tensor whose last dimension is a multiple of
    32; out: as fake_quant (may be x).  One read and one write per element."""
    _require_cuda(x, "x")
    if x.dim() < 1 or int(x.shape[-1]) % MX_BLOCK:
        raise _hip.DipoorletHipError(f"hadamard32: the last dimension must be a multiple of {MX_BLOCK}, got shape {list(x.shape)}")
    if out is None:
        y = torch.empty_like(x)
    else:
        _require_cuda(out, "out")
        if out.shape != x.shape or out.device != x.device:
            raise _hip.DipoorletHipError("hadamard32: out must have x's shape and device")
        y = out
    k = int(x.shape[-1])
    _hip.check(_hip.lib().dpl_hadamard32(_ptr(x), _ptr(y), x.numel() // k if k else 0, k, _stream()), "dpl_hadamard32")
    return y


GPTQ_FMT = {"int": _hip.GRID_UNIFORM, "e4m3": _hip.GRID_E4M3}     # include/dipoorlet_hip.h DPL_GRID_*
GPTQ_MAX_BLOCK = _hip.GPTQ_MAX_BLOCK
GptqGrid = collections.namedtuple("GptqGrid", "fmt scale zero_point qlo qhi", defaults=(None, 0, 0))
GptqGrid.__doc__ = """The grid GPTQ rounds onto: fmt 'int' (scale fp32 [1] or [rows], zero_point int32 of the same length, qlo < qhi: the
Q/DQ pair of fake_quant) or 'e4m3' (scale only: fake_quant_fp8)."""


def gptq_block(w, c0, nb, u, grid, err=None):
    """One block of GPTQ's column recursion, in place (dpl_gptq_block; tests/gptq_model.py gptq_block is the definition, matched
    bit for bit): columns [c0, c0 + nb) of w (fp32 [rows, K], one output channel per row) are rounded onto `grid` one after the
    other, each column's error e = (w - q) / u[c, c] going onto the block's later columns as w[:, k] -= e * u[c, k].  u: fp32
    [K', K'] (K' >= c0 + nb), the upper Cholesky factor of the inverse Hessian.  -> err fp32 [rows, nb].  1 <= nb <= 128."""
    _require_cuda(w, "w")
    _require_cuda(u, "u")
    if w.dim() != 2 or u.dim() != 2 or u.device != w.device:
        raise _hip.DipoorletHipError("gptq_block: w and u must be matrices on one device")
    if grid.fmt not in GPTQ_FMT:
        raise _hip.DipoorletHipError(f"gptq_block: grid.fmt must be 'int' or 'e4m3', got {grid.fmt!r}")
    rows = int(w.shape[0])
    if int(c0) < 0 or int(c0) + int(nb) > int(u.shape[0]):       # (the C ABI checks the columns of w and u; it cannot see u's rows)
        raise _hip.DipoorletHipError(f"gptq_block: rows [{c0}, {int(c0) + int(nb)}) lie outside u ({u.shape[0]} rows)")
    scale = grid.scale.to(device=w.device, dtype=torch.float32).contiguous().reshape(-1)
    zp = None
    if grid.fmt == "int":
        if grid.zero_point is None:
            raise _hip.DipoorletHipError("gptq_block: the integer grid needs a zero point")
        zp = grid.zero_point.to(device=w.device, dtype=torch.int32).contiguous().reshape(-1)
        if zp.numel() != scale.numel():
            raise _hip.DipoorletHipError("scale and zero_point lengths differ")
    if err is None:
        err = torch.empty((rows, max(int(nb), 0)), dtype=torch.float32, device=w.device)
    else:
        _require_cuda(err, "err")
        if err.device != w.device or err.numel() != rows * int(nb):
            raise _hip.DipoorletHipError("gptq_block: err must hold [rows, nb] elements on w's device")
    _hip.check(_hip.lib().dpl_gptq_block(_ptr(w), rows, int(w.shape[1]), int(c0), int(nb), _ptr(u), int(u.shape[1]), _ptr(scale),
                                         None if zp is None else _ptr(zp), scale.numel(), int(grid.qlo), int(grid.qhi),
                                         GPTQ_FMT[grid.fmt], _ptr(err), _stream()), "dpl_gptq_block")
    return err


def gptq_nearest(w, grid):
    """w (fp32 [rows, K]) rounded to nearest on `grid`, per-row parameters along axis 0: what GPTQ's result is measured against."""
    axis = 0 if grid.scale.numel() > 1 else None
    if grid.fmt == "int":
        return fake_quant(w, grid.scale, grid.zero_point, grid.qlo, grid.qhi, axis=axis)
    return fake_quant_fp8(w, grid.scale, axis=axis)


def gptq_quantize(w, u, grid, block=GPTQ_MAX_BLOCK):
    """GPTQ over a whole layer (tests/gptq_model.py gptq_layer32): the blocks left to right through gptq_block, and between them
    W[:, c0 + nb:] -= Err @ U[c0:c0 + nb, c0 + nb:], one fp32 GEMM of the BLAS library (the only step whose summation order is not
    this library's).  w: fp32 [rows, K] (not modified), u: fp32 [K, K].  -> (the rounded weight, Err [rows, K])."""
    _require_cuda(w, "w")
    _require_cuda(u, "u")
    if w.dim() != 2 or tuple(u.shape) != (w.shape[1], w.shape[1]):
        raise _hip.DipoorletHipError("gptq_quantize: w must be [rows, K] and u [K, K]")
    if not 1 <= int(block) <= GPTQ_MAX_BLOCK:
        raise _hip.DipoorletHipError(f"gptq_quantize: block must be in [1, {GPTQ_MAX_BLOCK}]")
    grid = grid._replace(scale=grid.scale.to(device=w.device, dtype=torch.float32),
                         zero_point=None if grid.zero_point is None else grid.zero_point.to(device=w.device, dtype=torch.int32))
    wq = w.clone()
    K = int(w.shape[1])
    err = torch.empty_like(wq)
    for c0 in range(0, K, int(block)):
        nb = min(int(block), K - c0)
        e = gptq_block(wq, c0, nb, u, grid)
        err[:, c0:c0 + nb] = e
        if c0 + nb < K:
            wq[:, c0 + nb:].addmm_(e, u[c0:c0 + nb, c0 + nb:], alpha=-1.0)
    return wq, err


def gptq_mx_block(w, c0, nb, u, elem, err=None, scales=None):
    """One call of GPTQ's column recursion on an MX block-scaled grid, in place (dpl_gptq_mx_block; tests/mx_gptq_model.py
    gptq_mx_block is the definition, matched bit for bit): gptq_block with the grid of every block of 32 columns fixed when the
    recursion enters it — the floor rule's shared exponent of the block's CURRENT values — and its columns rounded to `elem`
    ('mxfp8' / 'mxfp4') under it, saturating.  w: contiguous fp32 [rows, K]; whole blocks only: c0 a multiple of 32, nb (1 .. 128) one
    too unless c0 + nb == K.  -> (err fp32 [rows, nb], scales uint8 [rows, ceil(K / 32)]: the entry bytes of the call's blocks in
    their columns; a tensor passed as scales= keeps every other column)."""
    _require_cuda(w, "w")
    _require_cuda(u, "u")
    if elem not in MX_ELEM_MIXED:
        raise _hip.DipoorletHipError(f"gptq_mx_block: elem must be 'mxfp8' or 'mxfp4' (the recursion is held to these two grids), got {elem!r}")
    if w.dim() != 2 or u.dim() != 2 or u.device != w.device:
        raise _hip.DipoorletHipError("gptq_mx_block: w and u must be matrices on one device")
    rows, k = int(w.shape[0]), int(w.shape[1])
    if int(c0) < 0 or int(c0) + int(nb) > int(u.shape[0]):       # (the C ABI checks the columns of w and u; it cannot see u's rows)
        raise _hip.DipoorletHipError(f"gptq_mx_block: rows [{c0}, {int(c0) + int(nb)}) lie outside u ({u.shape[0]} rows)")
    nblk = -(-k // MX_BLOCK)
    if err is None:
        err = torch.empty((rows, max(int(nb), 0)), dtype=torch.float32, device=w.device)
    else:
        _require_cuda(err, "err")
        if err.device != w.device or err.numel() != rows * int(nb):
            raise _hip.DipoorletHipError("gptq_mx_block: err must hold [rows, nb] elements on w's device")
    if scales is None:
        scales = torch.zeros((rows, nblk), dtype=torch.uint8, device=w.device)
    elif not (isinstance(scales, torch.Tensor) and scales.is_cuda and scales.device == w.device and scales.dtype == torch.uint8
              and scales.is_contiguous() and tuple(scales.shape) == (rows, nblk)):
        raise _hip.DipoorletHipError(f"gptq_mx_block: scales must be a contiguous uint8 device tensor of shape [{rows}, {nblk}] on w's device")
    _hip.check(_hip.lib().dpl_gptq_mx_block(MX_ELEM[elem], _ptr(w), rows, k, k, int(c0), int(nb), _ptr(u), int(u.shape[1]), _ptr(err),
                                            _ptr(scales), nblk, _stream()), "dpl_gptq_mx_block")
    return err, scales


def gptq_mx_nearest(w, elem):
    """w (fp32 [rows, K]) rounded to nearest on the MX grid of its own blocks along K: what gptq_mx_quantize is measured against,
    and what the graph's MX node makes of an untouched weight."""
    return fake_quant_mx(w, 1, elem)


def gptq_mx_quantize(w, u, elem, block=GPTQ_MAX_BLOCK):
    """GPTQ over a whole layer on an MX grid (tests/mx_gptq_model.py gptq_mx_layer32): the calls left to right through
    gptq_mx_block, and between them W[:, c0 + nb:] -= Err @ U[c0:c0 + nb, c0 + nb:], one fp32 GEMM of the BLAS library.  w: fp32
    [rows, K], finite (not modified), u: fp32 [K, K]; block: columns per call, a multiple of 32 in [32, 128].  -> (the rounded
    weight — a fixed point of fake_quant_mx(., 1, elem) —, Err [rows, K], the entry bytes uint8 [rows, ceil(K / 32)])."""
    _require_cuda(w, "w")
    _require_cuda(u, "u")
    if w.dim() != 2 or tuple(u.shape) != (w.shape[1], w.shape[1]):
        raise _hip.DipoorletHipError("gptq_mx_quantize: w must be [rows, K] and u [K, K]")
    block = int(block)
    if block % MX_BLOCK or not MX_BLOCK <= block <= GPTQ_MAX_BLOCK:
        raise _hip.DipoorletHipError(f"gptq_mx_quantize: block must be a multiple of {MX_BLOCK} in [{MX_BLOCK}, {GPTQ_MAX_BLOCK}], got {block}")
    if not bool(torch.isfinite(w).all()):
        raise _hip.DipoorletHipError("gptq_mx_quantize: w holds a NaN or an infinity")
    wq = w.contiguous().clone()
    K = int(w.shape[1])
    err = torch.empty_like(wq)
    scales = torch.zeros((int(w.shape[0]), -(-K // MX_BLOCK)), dtype=torch.uint8, device=w.device)
    for c0 in range(0, K, block):
        nb = min(block, K - c0)
        e, _ = gptq_mx_block(wq, c0, nb, u, elem, scales=scales)
        err[:, c0:c0 + nb] = e
        if c0 + nb < K:
            wq[:, c0 + nb:].addmm_(e, u[c0:c0 + nb, c0 + nb:], alpha=-1.0)
    return wq, err, scales


class FakeQuantSet:
    """Fused QuantizeLinear -> DequantizeLinear over a WHOLE tensor set in one launch (dpl_fake_quant_items): for a caller that
    holds every tensor of a forward (the profiling flow's fp-vs-quantised comparison, quant_acti over a set) — one launch
    instead of one per Q/DQ pair, most of which are launch-bound.

        fq = FakeQuantSet(plan, params)          # params[t] = (scale fp32 [1 | C], zero_point int32 [1 | C], inner, qlo, qhi)
        ys = fq(xs)                              # or fq(xs, out=ys); xs[t]: [B, ...] contiguous fp32 as the plan describes

    `inner` = elements per channel row of ONE tensor as laid out in memory ([B, C, H, W] with per-channel parameters on axis 1:
    inner = H * W); ignored for per-tensor parameters.

    fmt='fp8': the OCP FP8 E4M3 grid (dpl_fake_quant_fp8_items, fake_quant_fp8) — params[t] = (scale fp32 [1 | C], inner)."""

    def __init__(self, plan, params, fmt="int"):
        if fmt not in ("int", "fp8"):
            raise _hip.DipoorletHipError(f"FakeQuantSet: fmt must be 'int' or 'fp8', got {fmt!r}")
        self.fmt = fmt
        if len(params) != plan.T:
            raise _hip.DipoorletHipError(f"expected {plan.T} parameter rows, got {len(params)}")
        self.plan = plan
        self.keep = []
        rows = (_hip.FakeQuantParams * plan.T)()
        for t, row in enumerate(params):
            if fmt == "fp8":
                scale, inner = row
                scale = scale.to(device=plan.device, dtype=torch.float32).contiguous().reshape(-1)
                self.keep.append(scale)
                rows[t] = _hip.FakeQuantParams(scale.data_ptr(), None, scale.numel(), int(inner) if scale.numel() > 1 else 1, 0, 0)
                continue
            scale, zp, inner, qlo, qhi = row
            scale = scale.to(device=plan.device, dtype=torch.float32).contiguous().reshape(-1)
            zp = zp.to(device=plan.device, dtype=torch.int32).contiguous().reshape(-1)
            if scale.numel() != zp.numel():
                raise _hip.DipoorletHipError("scale and zero_point lengths differ")
            self.keep += [scale, zp]
            rows[t] = _hip.FakeQuantParams(scale.data_ptr(), zp.data_ptr(), scale.numel(), int(inner) if scale.numel() > 1 else 1,
                                           int(qlo), int(qhi))
        self.d_params = _upload_struct_array(rows, plan.T, plan.device)
        # the balanced partition over the batch's tensors (slot = tensor): 65536 workgroups of ~52 KB on the ResNet-50 set, so
        # that the resident ones read and write a dense window as the dispatcher hands them out (measured: with
        # 1024 resident workgroups of 3.3 MB each the read + write stream reaches 0.73 of 8 TB/s on some boxes of the pool and
        # 0.60 - 0.62 on others; 65536: 0.70 - 0.73 on both kinds)
        self.work = plan.work("fq")

    def __call__(self, tensors, out=None):
        plan = self.plan
        tx = plan.seg_table(tensors)
        if out is None:
            out = [torch.empty_like(x) for x in tensors]
        ty = plan.seg_table(out)
        entry = "dpl_fake_quant_fp8_items" if self.fmt == "fp8" else "dpl_fake_quant_items"
        _hip.check(getattr(_hip.lib(), entry)(*self.work.args(), _ptr(tx), _ptr(ty), _ptr(self.d_params), _stream()), entry)
        return out


def cos_accumulate(a, b, acc, slot=0):
    """acc[slot] += (sum a*b, sum a*a, sum b*b) in fp64 (utils.py:273-278 partial sums)."""
    _require_cuda(a, "a")
    _require_cuda(b, "b")
    if a.numel() != b.numel():
        raise _hip.DipoorletHipError("cos_accumulate: size mismatch")
    # (the kernel adds three fp64 values at acc + 3 * slot: a slot the accumulator does not hold would be written past its end)
    if not (isinstance(acc, torch.Tensor) and acc.device == a.device and acc.dtype == torch.float64 and acc.is_contiguous()):
        raise _hip.DipoorletHipError("cos_accumulate: acc must be a contiguous fp64 tensor on a's device")
    if not 0 <= int(slot) < acc.numel() // 3:
        raise _hip.DipoorletHipError(f"cos_accumulate: slot {slot} outside an accumulator of {acc.numel() // 3} slots")
    _hip.check(_hip.lib().dpl_cos_accumulate(_ptr(a), _ptr(b), a.numel(), _ptr(acc), slot, _stream()),
               "dpl_cos_accumulate")
    return acc


def channel_diff_sum(a, b, acc=None):
    """acc[c] += sum over every axis but the channel one of (a - b), fp64 (bias_correction.py:9-13).
    a, b: [n, C, spatial...] (channel axis 1) or [n, C]; returns the fp64 device tensor [C]."""
    _require_cuda(a, "a")
    _require_cuda(b, "b")
    if a.shape != b.shape or a.dim() < 2:
        raise _hip.DipoorletHipError("channel_diff_sum: shapes must match and carry a channel axis")
    n_ch = int(a.shape[1])
    inner = 1
    for d in a.shape[2:]:
        inner *= int(d)
    if acc is None:
        acc = torch.zeros(n_ch, dtype=torch.float64, device=a.device)
    # (the kernel adds C fp64 values at acc: anything smaller, of another type or strided would be written past or between)
    elif not (isinstance(acc, torch.Tensor) and acc.device == a.device and acc.dtype == torch.float64 and acc.is_contiguous()
              and acc.numel() == n_ch):
        raise _hip.DipoorletHipError(f"channel_diff_sum: acc must be a contiguous fp64 tensor of {n_ch} elements on a's device")
    _hip.check(_hip.lib().dpl_channel_diff_sum(_ptr(a), _ptr(b), int(a.shape[0]), n_ch, inner, _ptr(acc), _stream()),
               "dpl_channel_diff_sum")
    return acc


GEMM_SMALL_MAX = 1 << 28      # DPL_GEMM_SMALL_MAX (include/dipoorlet_hip.h)


def gemm_small(a, b, bias=None, alpha=1.0, beta=1.0):
    """alpha * a @ b + beta * bias through dpl_gemm_small (csrc/gemm_small.hip: the classifier head of a convolutional network,
    so that a calibration run of one never initialises torch's BLAS path).  a: [M, K] fp32 contiguous; b: [K, N] fp32, any strides (a transposed
    view of an [N, K] weight is what an ONNX Gemm with transB = 1 gives); bias: None, [N], [1, N], [M, 1] or [M, N].
    M * N * K <= GEMM_SMALL_MAX."""
    for t, name in ((a, "a"), (b, "b")) + (((bias, "bias"),) if bias is not None else ()):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise _hip.DipoorletHipError(f"gemm_small: {name} must be a ROCm device tensor; dipoorlet_amd has no CPU path")
        if t.dtype != torch.float32:
            raise _hip.DipoorletHipError(f"gemm_small: {name} must be float32")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
        raise _hip.DipoorletHipError("gemm_small: a [M, K] and b [K, N]")
    a = a.contiguous()
    M, K, N = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    bp, sm, sn = None, 0, 0
    if bias is not None:
        bias = bias.expand(M, N)       # (broadcast axes get stride 0; raises if it does not broadcast)
        bp, sm, sn = _ptr(bias), int(bias.stride(0)), int(bias.stride(1))
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    L = _hip.lib()
    need = int(L.dpl_gemm_small_workspace(M, N, K))
    ws = torch.empty(need // 4, dtype=torch.float32, device=a.device) if need else None
    _hip.check(L.dpl_gemm_small(_ptr(a), _ptr(b), bp, _ptr(out), M, N, K, int(b.stride(0)), int(b.stride(1)), sm, sn,
                                float(alpha), float(beta), _ptr(ws) if need else None, _stream()), "dpl_gemm_small")
    return out


def cos_per_image(plan, tensors_a, tensors_b):
    """Cosine partial sums for every (image, tensor) pair of two tensor sets with the same geometry ->
    fp64 device tensor [B, T, 3] = (sum a*b, sum a*a, sum b*b)."""
    w = plan.work("cos", per_image=True)
    ta = plan.seg_table(tensors_a)
    tb = plan.seg_table(tensors_b)
    acc = torch.zeros(plan.batch, plan.T, 3, dtype=torch.float64, device=plan.device)
    _hip.check(_hip.lib().dpl_cos_items_accumulate(*w.args(), _ptr(ta), _ptr(tb), _ptr(acc), _stream()),
               "dpl_cos_items_accumulate")
    return acc
