/*
 * dipoorlet_hip.h — C ABI of the MI355X (gfx950) activation-calibration core.
 *
 * Drop-in boundary for Dipoorlet's calibration hot path.  The reference has no native layer: the
 * arithmetic below is what its Python does with numpy on host copies of every activation
 * (citations are into the reference tree, dipoorlet/...).  Each entry point names the reference
 * code it replaces.  All device work is enqueued on the caller's HIP stream, never synchronises,
 * never allocates; every buffer is caller-owned device memory unless marked HOST.
 *
 * Conventions
 *   - return value: 0 = ok, negative = error; dpl_last_error() gives a thread-local message.
 *   - "slot"  : index of an accumulator (one per calibrated tensor, or per (image,tensor) pair).
 *   - "seg"   : index into a device table of base pointers (one per live activation tensor).
 *   - "span"  : `count` consecutive fp32 elements at `offset` inside a segment, feeding one slot.
 *   - spans are cut into work items (one workgroup each) by dpl_build_work_items().
 *   - fp32 min/max accumulators are kept order-encoded in uint32 so integer atomics apply:
 *         enc(f) = bits(f) ^ (bits(f) >> 31 ? 0xFFFFFFFF : 0x80000000)
 */
#ifndef DIPOORLET_HIP_H
#define DIPOORLET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPL_ABI_VERSION 36 /* 20: dpl_fake_quant_pre (the producer's ReLU / Add + ReLU inside the Q/DQ kernel); 21: dpl_stream_*; 22: dpl_hist_kl;
                              23: dpl_minmax_hist_accumulate / dpl_hist_spec_* (a batch's histogram taken in the range pass);
                              24: dpl_fake_quant_fp8 / dpl_fake_quant_fp8_items (the Q/DQ pair on the OCP FP8 E4M3 grid);
                              25: dpl_hist_qmse (quantisation-MSE clip search on the integer or the E4M3 grid);
                              26: dpl_colwise_absmax (per-channel running max |x| of a channels-last activation: --smooth);
                              27: dpl_fake_quant_mx (the OCP Microscaling Q/DQ pair, MXFP8 / MXFP4: --mx);
                              28: dpl_gptq_block (sequential quantise-and-compensate of a block of weight columns: --gptq);
                              29: dpl_hadamard32 (32-point Hadamard rotation of every MX block of an activation: --mx_rotate);
                              30: dpl_mx_encode / dpl_mx_decode (an MX tensor as packed element codes and E8M0 scale bytes: --mx_pack);
                              31: dpl_mx_gemm (two packed MX operands through CDNA4's block-scaled matrix instruction: --mx_verify);
                              32: dpl_mx_scale_search / dpl_fake_quant_mx_scaled / dpl_mx_encode_scaled (error-minimising E8M0 scales
                                  for constant MX operands, and the Q/DQ and the packed bytes under given scales: --mx_scale_search);
                              33: dpl_gptq_mx_block (dpl_gptq_block's recursion on the MX block-scaled grids: --mx_gptq);
                              34: dpl_mx_conv (a convolution of two packed MX operands on the block-scaled matrix instruction: --mx_conv);
                              35: dpl_mx_gemm_err (dpl_mx_gemm's product against a reference, as per-tile fp64 error sums: --mx_mixed);
                              36: DPL_MX_E2M3 / DPL_MX_E3M2 (the two OCP MXFP6 element formats, through the MX entry points there are) */
#define DPL_MAX_BINS 16384 /* LDS-privatised histogram: bins * 4 B per workgroup */
#define DPL_HIST_SPEC_MAX_TENSORS 2048 /* dpl_hist_spec_accumulate keeps a prefix sum over the tensors in LDS */

typedef void* dpl_stream_t; /* hipStream_t */

typedef struct dpl_span {
    uint64_t offset; /* elements from the segment base */
    uint64_t count;  /* elements */
    uint32_t seg;
    uint32_t slot;
} dpl_span;

typedef struct dpl_work_item {
    uint64_t offset;
    uint32_t count;
    uint32_t seg;
    uint32_t slot;
    uint32_t reserved;
} dpl_work_item;

/* Per-slot histogram range, derived on device from the running min/max (np.histogram semantics,
 * forward_net.py:266-268): first/last outer edges, fp32 step, reciprocal for the index estimate. */
typedef struct dpl_hist_range {
    float first, last, step, inv;
    uint32_t zero_bin; /* bin that |x| == 0 falls in */
    uint32_t status;   /* 0 ok, 1 range not finite (numpy raises ValueError), 2 too many bins for range */
    float dmax;        /* max(gmax, -gmin) before the degenerate +-0.5 expansion */
    uint32_t exact_div; /* 1: use the correctly rounded divide for the index estimate */
} dpl_hist_range;

/* Per-(image,tensor) OCTAV state (forward_net.py:315-340). */
typedef struct dpl_octav_state {
    double sum;       /* sum |x| (first pass) / sum_{|x|>s} |x| */
    uint64_t cnt_gt;  /* count(|x|>0) (first pass) / count(|x|>s) */
    uint64_t cnt_le;  /* count(|x|<=s) */
    uint32_t min_enc, max_enc;
    uint32_t nan_seen;
    uint32_t done;
    float s;
    float unsigned_div; /* 1 or 4 */
    uint32_t iters;
    uint32_t mode;      /* 0: every evaluation re-reads the full data; 1: tail lists (dpl_octav_run_compact);
                           2: log-histogram bracket (dpl_octav_run_bracket) / one-read walk; 3: one-read rescue */
    uint64_t n_elems;   /* elements of the pair (counted by the first pass) */
    uint32_t len[2];    /* lengths of the two tail lists */
    uint32_t cur;       /* list holding the values above the previous iterate: 0, 1, or 2 = none yet */
    uint32_t reserved;  /* compaction route: float bits of the iterate the current tail list was built at */
} dpl_octav_state;

int dpl_abi_version(void);
const char* dpl_last_error(void);
/* 0 when the current HIP device is a gfx950 part; fills name (HOST buffer) when non-null. */
int dpl_device_info(char* name, int name_cap, int* compute_units, uint64_t* hbm_bytes);
/* A HIP stream of a given priority on the current device (hipStreamNonBlocking), for work that runs BESIDE a caller's stream: the
 * OCTAV pipeline's rescue / result kernels.  priority: what hipDeviceGetStreamPriorityRange reports — *greatest (-1: high) ...
 * *least (1: low) on gfx950; values outside the range are clamped.  A LOW-priority stream lives on a hardware queue of its own class:
 * it neither takes the workgroup slots the caller's streaming kernel is waiting for (a high-priority one does) nor shares a queue
 * with the caller's stream (a normal-priority one may, depending on the order the process created its streams: the two then run one
 * after the other).  torch cannot create one (it clamps priorities above 0 to 0): wrap the handle in torch.cuda.ExternalStream. */
int dpl_stream_priority_range(int* least, int* greatest);
int dpl_stream_create(int priority, dpl_stream_t* out);
int dpl_stream_destroy(dpl_stream_t s);

/* HOST-only: cut spans into work items of at most `chunk_elems` (multiple of 1024) elements.
 * Returns the number of items (may exceed cap: call again with a larger buffer), <0 on error. */
int64_t dpl_build_work_items(const dpl_span* spans, int64_t n_spans, uint64_t chunk_elems,
                             dpl_work_item* out, int64_t cap);
/* HOST-only: split the concatenated element stream of `spans` into n_blocks contiguous, equal shares
 * (cuts 4 KiB-aligned inside a span).  Writes the items in stream order and block_begin[0..n_blocks]
 * (workgroup b owns items [block_begin[b], block_begin[b+1])).  Returns the item count (call with
 * out = NULL to size the buffer).  Few large, equal shares stream faster from HBM than many small items. */
int64_t dpl_build_balanced_items(const dpl_span* spans, int64_t n_spans, int64_t n_blocks, dpl_work_item* out,
                                 int64_t cap, uint32_t* block_begin);

/* ---- running min / max: replaces ort_outs[i].max()/.min() per tensor per image
 *      (forward_net.py:220-235) and np.min/np.max over the per-image lists (basic_algorithm.py:21). */
int dpl_minmax_init(uint32_t* d_min_enc, uint32_t* d_max_enc, uint32_t* d_nan, int64_t n_slots, dpl_stream_t s);
/* d_block_begin: device copy of block_begin (n_blocks + 1 entries), or NULL with n_blocks == n_items. */
int dpl_minmax_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                          int64_t n_blocks, const float* const* d_seg_ptrs, uint32_t* d_min_enc,
                          uint32_t* d_max_enc, uint32_t* d_nan, dpl_stream_t s);
/* decode to fp32; a slot that saw a NaN yields NaN for both (numpy max/min propagate NaN). */
int dpl_minmax_finalize(const uint32_t* d_min_enc, const uint32_t* d_max_enc, const uint32_t* d_nan,
                        int64_t n_slots, float* d_min, float* d_max, dpl_stream_t s);
/* inverse of finalize for merged (e.g. all-reduced) fp32 ranges. */
int dpl_minmax_encode(const float* d_min, const float* d_max, int64_t n_slots, uint32_t* d_min_enc,
                      uint32_t* d_max_enc, uint32_t* d_nan, dpl_stream_t s);

/* ---- |x| histogram: replaces np.histogram(np.abs(x), int(bins), (0, data_max)) per tensor per image
 *      and the np.stack(hist).sum(0) (forward_net.py:265-280, basic_algorithm.py:37-38).
 *      Counts are bit-exact with numpy; d_hist is uint64 [n_slots, bins], accumulated in place. */
int dpl_hist_prepare(const float* d_min, const float* d_max, int64_t n_slots, int bins,
                     dpl_hist_range* d_ranges, dpl_stream_t s);
int dpl_abs_hist_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                            int64_t n_blocks, const float* const* d_seg_ptrs, const dpl_hist_range* d_ranges,
                            int bins, uint64_t* d_hist, dpl_stream_t s);
/* ---- the same histogram with the second read skipped where the range pass guessed the range right.  np.histogram's bins depend on the
 *      shard's final dmax alone (dpl_hist_range), and a tensor's running dmax stops moving once the batch holding its extreme has
 *      passed.  dpl_minmax_hist_accumulate is dpl_minmax_accumulate that ALSO histograms the batch against the range the accumulators
 *      give BEFORE the launch (a snapshot: dpl_minmax_finalize + dpl_hist_prepare of the running values, through the same device
 *      code) into a caller-owned ledger entry; dpl_hist_spec_accumulate is dpl_abs_hist_accumulate for a batch that has such an entry:
 *      d_hist[t, :] += the entry's row where the snapshot equals d_ranges[t] in all 32 bytes and its status is 0, the kernel of
 *      dpl_abs_hist_accumulate over the other tensors only (a balanced partition of what remains, derived on the device; no host
 *      round trip).  The counts are the ones dpl_abs_hist_accumulate gives, provided the batch's data did not change in between.
 *      d_entry: dpl_hist_spec_entry_bytes(n_slots, bins) bytes, 16-byte aligned:
 *          dpl_hist_range snapshot[n_slots] | uint32 flags[n_slots] | pad to 16 | uint32 counts[n_slots, bins]
 *      flags (written by dpl_hist_spec_accumulate): 1 = row added, the tensor was not read; 2 = status != 0, nothing to count; 0 = read.
 *      The items of dpl_minmax_hist_accumulate are any partition with slot < n_slots and fewer than 2^32 elements per slot.
 *      dpl_hist_spec_accumulate takes the per-tensor form: tensor t = segment t = slot t from offset 0, d_elems[t] (< 2^32) elements,
 *      n_slots <= DPL_HIST_SPEC_MAX_TENSORS, n_blocks workgroups.  d_stats (may be NULL): uint64 [4] += {tensors, tensors not read,
 *      elements, elements not read}. */
uint64_t dpl_hist_spec_entry_bytes(int64_t n_slots, int bins);
int dpl_minmax_hist_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                               int64_t n_blocks, const float* const* d_seg_ptrs, uint32_t* d_min_enc, uint32_t* d_max_enc,
                               uint32_t* d_nan, int64_t n_slots, int bins, void* d_entry, dpl_stream_t s);
int dpl_hist_spec_accumulate(void* d_entry, const uint64_t* d_elems, int64_t n_slots, int64_t n_blocks,
                             const float* const* d_seg_ptrs, const dpl_hist_range* d_ranges, int bins, uint64_t* d_hist,
                             uint64_t* d_stats, dpl_stream_t s);
/* TEST HOOK, not part of the stable interface (it may change or go with the kernel it describes): the cuts
 * dpl_hist_spec_accumulate's kernel works to for the flags the entry holds now — d_cuts uint64 [n_blocks + 1],
 * positions in the stream of the tensors still to be read (flags == 0), d_cuts[n_blocks] = its length. */
int dpl_hist_spec_cuts(const void* d_entry, const uint64_t* d_elems, int64_t n_slots, int64_t n_blocks, uint64_t* d_cuts,
                       dpl_stream_t s);
/* ---- percentile clip: replaces the python loop of basic_algorithm.py:40-53. d_clip: fp32 [n_slots,2]. */
int dpl_hist_percentile(const uint64_t* d_hist, const float* d_min, const float* d_max, int64_t n_slots,
                        int bins, double threshold, float* d_clip, dpl_stream_t s);

/* ---- entropy (KL-divergence) clip on the same histogram: beyond the reference, which names "kl" in its --bins help and never
 *      shipped one.  For every candidate i in [levels, bins] (keep bins [0, i), outliers folded into bin i - 1) the divergence
 *      between the kept histogram and its image on `levels` groups, both smoothed with eps = 1e-4; the clip is the centre of bin
 *      i* - 1 for the lowest i* of least divergence, in fp32 as dpl_hist_percentile ends.  The definition is tests/kl_model.py.
 *      d_div fp64 [n_slots, bins + 1] is caller-provided workspace AND output (the divergence of every candidate, +inf where not
 *      admissible or i < levels); d_best int32 [n_slots] (i*, -1: none -> the clip is [min, max]); d_clip fp32 [n_slots, 2].
 *      2 <= levels <= bins <= DPL_MAX_BINS.  No floating-point atomics: two calls give the same bits. */
int dpl_hist_kl(const uint64_t* d_hist, const float* d_min, const float* d_max, int64_t n_slots, int bins,
                int levels, double* d_div, int32_t* d_best, float* d_clip, dpl_stream_t s);

/* ---- quantisation-MSE clip on the same histogram, on the platform's own grid: beyond the reference, whose "mse" is OCTAV (a
 *      per-image fixed point).  In units of half a bin width: bin b's centre is m = 2 b + 1, candidate i in [first, bins] clips at
 *      t = 2 i - 1 (the centre of bin i - 1) with scale t / top; u = m top / t, Q = the grid point nearest to min(u, top), and
 *      err[i] = (t / (2 top))^2 sum_b h[b] (u - Q)^2 / N: the mean squared error of the fake-quantised bin centres, in bin
 *      widths^2.  grid = DPL_GRID_UNIFORM: the integers 0 .. top, 1 <= top <= 32767 (127 for 8 bits); DPL_GRID_E4M3: the 127
 *      non-negative finite OCP FP8 E4M3 codes, largest 448, and `top` must be 0.  The clip is the centre of bin i* - 1 for the
 *      lowest i* of least error, in fp32 as dpl_hist_percentile ends.  The definition is tests/qmse_model.py.
 *      d_err fp64 [n_slots, bins + 1] is caller-provided workspace AND output (+inf for i < first, and everywhere for an empty
 *      histogram); d_best int32 [n_slots] (i*, -1: none -> the clip is [min, max]); d_clip fp32 [n_slots, 2].
 *      1 <= first <= bins <= DPL_MAX_BINS.  No floating-point atomics: two calls give the same bits. */
#define DPL_GRID_UNIFORM 0
#define DPL_GRID_E4M3 1
int dpl_hist_qmse(const uint64_t* d_hist, const float* d_min, const float* d_max, int64_t n_slots, int bins,
                  int first, int grid, int top, double* d_err, int32_t* d_best, float* d_clip, dpl_stream_t s);

/* ---- OCTAV ("mse"): replaces forward_net.py:315-330 per (image,tensor) pair (slot = pair).
 *      dpl_octav_run enqueues the first pass plus 20 (pass, update) rounds; converged pairs exit early. */
/* d_states holds n_pairs + 1 entries: the last one is a control block (count of pairs in full-pass mode). */
int dpl_octav_init(dpl_octav_state* d_states, int64_t n_pairs, int list_mode, dpl_stream_t s);
int dpl_octav_run(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin, int64_t n_blocks,
                  const float* const* d_seg_ptrs, dpl_octav_state* d_states, int64_t n_pairs, int dynamic_sym,
                  int max_iters, dpl_stream_t s);
/* Same iterate sequence with tail compaction (init with list_mode = 1): the first evaluation reads the data
 * once and writes the values above s_0 to d_list0; then ONE launch walks all remaining iterations with a
 * persistent workgroup per pair over the shrinking tail lists (~2.5x smaller per step).
 * d_pair_spans[pair] = where the pair's data lives (seg, offset, count); d_pair_base[pair] = element offset of
 * the pair's region in both lists (a region holds the pair's element count); d_pair_order = pair indices,
 * largest first (launch order of the per-pair workgroups), may be NULL.  Pairs whose iterate decreases
 * (degenerate data) finish on the full data. */
int dpl_octav_run_compact(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                          int64_t n_blocks, const float* const* d_seg_ptrs, dpl_octav_state* d_states,
                          int64_t n_pairs, const dpl_span* d_pair_spans, const uint64_t* d_pair_base,
                          const uint32_t* d_pair_order, float* d_list0, float* d_list1, int dynamic_sym,
                          int max_iters, dpl_stream_t s);
/* Same iterate sequence in TWO reads of the data and no tail lists (init with list_mode = 2): pass 1 takes the
 * statistics and an exact log-scale histogram of |x| (64 bins per octave over 2^-18..2^14: per bin a count
 * and an integer sum of mantissas); a per-pair bracket walk over the bin edges marks the few dozen bins the
 * iterates can visit; pass 2 gathers only those elements (about 2 %) into d_list0; a per-pair kernel then runs the
 * exact iteration from (exact totals of the bins above) + (gathered elements of the current bin), verifying
 * that every iterate lands in a marked bin.  Pairs it cannot serve (bracket explodes on flat / degenerate
 * distributions, values >= 2^14, failed verification) are finished by the compaction route above.
 * d_lh_cnt: uint32 [n_pairs, 2048]; d_lh_sum: uint64 [n_pairs, 2048] (scratch: after the bracket walk they hold the
 * suffix totals N_ge[j] / S_ge[j] (fp64 bits) the exact walk reads); d_bitmap: uint32 [n_pairs, 66]
 * (64 words of marks + the gathered value range as two float bit patterns). */
int dpl_octav_run_bracket(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                          int64_t n_blocks, const float* const* d_seg_ptrs, dpl_octav_state* d_states,
                          int64_t n_pairs, const dpl_span* d_pair_spans, const uint64_t* d_pair_base,
                          const uint32_t* d_pair_order, float* d_list0, float* d_list1, uint32_t* d_lh_cnt,
                          uint64_t* d_lh_sum, uint32_t* d_bitmap, int dynamic_sym, int max_iters, dpl_stream_t s);
/* The reference's result in ONE read of the data and one launch per batch — the EXACT-TAIL form (csrc/octav_tail.hpp, included by
 * csrc/octav_tail_host.hip; replaces forward_net.py:323-330's 21 numpy passes):
 *   k_octav_tail — one workgroup per SLICE (at most dpl_octav_slice_cap() elements of one (image, tensor) pair; all but the largest
 *     pairs are one slice): the slice's only HBM read yields min / max, an exact log-scale histogram of |x| in LDS (64 bins per
 *     octave over 2^-18 .. 2^14: per bin a count and an integer mantissa sum) and the LIST of the values at or above a threshold
 *     bin (per tensor: the lowest bin its pairs asked for in the last two epochs of batches — a pair asks for the bin above which
 *     1/256 of it lies —, raised on the fly by a wave that lists more than its budget: ~0.5 - 1.5 % of a pair); then the same
 *     workgroup WALKS the pair: the early iterates as LOWER BOUNDS from the histogram's suffix totals, the late ones exactly from the
 *     list; accepted only if it ends on two exact evaluations;
 *   k_octav_tail_merge — a pair of more than one slice: its slices are streamed like pairs (packed histogram row per slice in d_lh),
 *     one workgroup adds the rows up, moves the lists together and runs the same walk;
 *   the RESCUE of a refused pair, on the device and without the host: the walk forms the pair's exact bracket from its histogram
 *     and puts the pair on a work list (d_missed); k_octav_rescue_gather re-reads THOSE PAIRS ALONE (many workgroups per pair) for
 *     the bracket's bins, k_octav_walk_rescue walks every iterate of the reference's sequence, verified; what even that cannot
 *     finish (a bracket that cannot be formed: flat distributions, values >= 2^14; a list beyond its region) ends on the
 *     compaction route (dpl_octav_oneread_compaction).  The rescue kernels are launched behind every batch and return at once
 *     when the control block (d_states[n_pairs]) lists nothing.
 * (Rounds 2 - 3 listed the bins ALL iterates were predicted to visit and evaluated every iterate exactly — k_octav_oneread,
 * k_octav_probe, k_octav_sort, k_octav_walk[_sorted]: superseded in round 4, removed in round 5.)
 *   dpl_build_octav_slices (HOST): cuts every span (= pair), largest first, into ceil(count / cap) equal slices (multiples
 *     of 4 elements); item.reserved = the pair's slice count; pair_slice0[2 slot], [2 slot + 1] = first / one-past-last
 *     slice of the pair in slot `slot` (spans carry slots 0 .. n_spans-1).  Returns the slice count (call with out = NULL
 *     to size), -3 when a pair needs more than 64 slices (use dpl_octav_run_bracket for such a set).
 * One HOST struct carries a batch's buffers (all pointers are device pointers; dpl_octav_plan_bind below fills it):
 *   dpl_octav_oneread_prepare = state initialisation (no dpl_octav_init call) + the tensors' threshold snapshot;
 *   dpl_octav_oneread_stream  = k_octav_tail (+ k_octav_tail_merge);
 *   dpl_octav_oneread_finish  = the rescue (+ dpl_octav_oneread_compaction when job.compaction_inline);
 *   dpl_octav_run_oneread = all of them on one stream.
 * stream and finish may run on different streams (the rescue of batch i beside the streaming kernel of batch i + 1) when the
 * caller orders finish(i) after stream(i) and gives concurrently live batches their own d_states / d_pred / d_lh / d_rescue_bm /
 * d_missed / d_resc; d_vis is shared (maxima are only ever raised), d_list0 may be shared by batches whose stream calls are on
 * one stream, d_list1 by batches whose finish calls are on one stream. */
typedef struct dpl_octav_oneread_job {
    /* the tensor set's decomposition (static per plan) */
    const dpl_work_item* d_slices;   /* dpl_build_octav_slices */
    int64_t n_slices;
    const uint32_t* d_pair_slice0;   /* [n_pairs, 2] */
    const dpl_span* d_pair_spans;    /* [n_pairs]: where each pair's data lives */
    const uint64_t* d_pair_base;     /* [n_pairs + 1]: element offset of the pair's region in d_list0 / d_list1; a region holds
                                        d_pair_base[p + 1] - d_pair_base[p] = dpl_octav_list_cap(elements) values (a pair of c slices:
                                        c x dpl_octav_list_cap(slice)), a multiple of 32 (a region must not share a 128-byte line with its
                                        neighbour: the streaming workgroup reads back the list it has just written); what a pair lists or
                                        its rescue gathers beyond that is dropped and the pair finishes on the compaction route */
    const uint32_t* d_pair_order;    /* [n_pairs]: pair indices, largest first (the pairs of more than one slice are its first n_multi entries) */
    int64_t n_pairs, n_tensors, n_small;   /* n_small: pairs of at most dpl_octav_small_pair() elements (they list their whole window) */
    int64_t n_multi;                 /* pairs of more than one slice */
    const dpl_work_item* d_items;    /* the balanced partition of the same pairs (compaction route), as for dpl_octav_run_compact */
    int64_t n_items;
    const uint32_t* d_block_begin;
    int64_t n_blocks;
    /* this batch */
    const float* const* d_seg_ptrs;
    dpl_octav_state* d_states;       /* [n_pairs + 1]; the last one is the control block: len[0] = pairs rescued, cnt_le = pairs left
                                        for the compaction route, sum = values listed */
    uint64_t* d_lh;                  /* [slices of multi-slice pairs, 2048]: a packed histogram row per such slice (may be NULL with n_multi == 0) */
    uint32_t* d_pred;                /* [n_tensors, 128]: the threshold snapshot (word 0 of a tensor's row) */
    float* d_list0;                  /* listed values, region per pair: written by dpl_octav_oneread_stream, dead once it has run */
    float* d_list1;                  /* the rescue's gathered values, same layout (dpl_octav_oneread_finish) */
    const uint64_t* d_pair_base_full;/* [n_pairs + 1]: whole-pair regions (element count rounded up to 32) ... */
    float* d_clist0;                 /* ... in the compaction route's two lists (dpl_octav_oneread_compaction): only needed once a batch */
    float* d_clist1;                 /*     reports unfinished pairs (d_states[n_pairs].cnt_le != 0), or up front with compaction_inline */
    uint32_t* d_rescue_bm;           /* [n_pairs, 64]: exact bracket of a rescued pair */
    uint32_t* d_missed;              /* [n_pairs, 3]: (pair, first unit, units) of the rescued pairs */
    uint64_t* d_resc;                /* [n_pairs, 3072]: suffix totals of a rescued pair (2048 fp64 sums, 2048 u32 counts): what its second walk starts from */
    /* carried across batches */
    uint32_t* d_vis;                 /* [2, n_tensors, 64] threshold history: two epoch accumulators (word 0 of a tensor's row: 2048 - the lowest
                                        bin its pairs asked for); walks raise d_vis[write_epoch], cleared first when reset_epoch != 0 */
    int32_t write_epoch, reset_epoch;
    int32_t dynamic_sym, max_iters;
    int32_t compaction_inline;       /* 1: dpl_octav_oneread_finish ends with dpl_octav_oneread_compaction; 0: the caller reads d_states[n_pairs].cnt_le
                                        when the batch is done and calls it only when that is non-zero */
    int32_t reserved;
} dpl_octav_oneread_job;
uint32_t dpl_octav_slice_cap(void);
uint32_t dpl_octav_list_cap(uint64_t n_elements); /* values the list region of a single-slice pair / of one slice of n elements holds */
uint32_t dpl_octav_small_pair(void); /* pairs of at most this many elements list their whole window */
int64_t dpl_build_octav_slices(const dpl_span* spans, int64_t n_spans, dpl_work_item* out, int64_t cap, uint32_t* pair_slice0);
int dpl_octav_oneread_prepare(const dpl_octav_oneread_job* job, dpl_stream_t s);
int dpl_octav_oneread_stream(const dpl_octav_oneread_job* job, dpl_stream_t s);
int dpl_octav_oneread_finish(const dpl_octav_oneread_job* job, dpl_stream_t s);
int dpl_octav_oneread_compaction(const dpl_octav_oneread_job* job, dpl_stream_t s);
int dpl_octav_run_oneread(const dpl_octav_oneread_job* job, dpl_stream_t s);

/* The exact-tail form WITHOUT knowing any buffer's size (what forward_net.py:315-340 needs from a binding): a HOST plan over the
 * (image, tensor) pairs of one tensor-set geometry reports the bytes of every part of the workspace, uploads its static tables
 * into caller memory and fills the job.  Minimal use, one batch at a time on one stream:
 *     p = dpl_octav_plan_create(spans, B * T, T, 1024);  dpl_octav_plan_sizes(p, &z);
 *     [hipMalloc z.tables_bytes, z.history_bytes (memset 0), z.state_bytes, z.rescue_bytes, 2 x z.list_bytes, z.fallback_bytes, z.result_bytes]
 *     dpl_octav_plan_upload(p, d_tables, s);
 *     per batch k: dpl_octav_plan_bind(p, d_tables, d_history, d_state, d_rescue, d_list0, d_list1, d_fallback, d_seg_ptrs, k, dyn, 20, &job);
 *                  dpl_octav_run_oneread(&job, s);  dpl_octav_finalize(job.d_states, job.n_pairs, d_result, s);
 * spans: one per pair, slot = image * n_tensors + tensor = its index.  NULL (dpl_last_error) when a pair needs more than 64
 * slices (dpl_octav_run_bracket serves such a set).  n_blocks: workgroups of the compaction route's partition (1024).
 * A pipeline that keeps several batches in flight gives each its own d_state / d_rescue, one d_list0 per stream that carries
 * dpl_octav_oneread_stream, one d_list1 per stream that carries dpl_octav_oneread_finish, and may pass d_fallback = NULL:
 * job.compaction_inline is then 0 and the caller binds a fallback block (z.fallback_bytes) only when it reads a non-zero
 * d_states[n_pairs].cnt_le, then calls dpl_octav_oneread_compaction + dpl_octav_finalize for that batch. */
typedef struct dpl_octav_plan dpl_octav_plan;
typedef struct dpl_octav_workspace_sizes {
    uint64_t tables_bytes;   /* the static decomposition (dpl_octav_plan_upload fills it) */
    uint64_t history_bytes;  /* what the tensors' pairs asked for in earlier batches: zero it once per calibration run, share it between the run's batches */
    uint64_t state_bytes;    /* per batch in flight: pair states + control block, the tensors' threshold snapshot */
    uint64_t rescue_bytes;   /* per batch in flight: brackets, work list and suffix totals of rescued pairs, histogram rows of multi-slice pairs */
    uint64_t list_bytes;     /* ONE list buffer; a job takes two (d_list0, d_list1) */
    uint64_t fallback_bytes; /* the compaction route's two whole-pair lists */
    uint64_t result_bytes;   /* fp32 [n_pairs, 3] of dpl_octav_finalize */
    int64_t n_pairs, n_slices, n_multi, n_small;
} dpl_octav_workspace_sizes;
dpl_octav_plan* dpl_octav_plan_create(const dpl_span* spans, int64_t n_spans, int64_t n_tensors, int64_t n_blocks);
void dpl_octav_plan_destroy(dpl_octav_plan* plan);
int dpl_octav_plan_sizes(const dpl_octav_plan* plan, dpl_octav_workspace_sizes* out);
int dpl_octav_plan_upload(const dpl_octav_plan* plan, void* d_tables, dpl_stream_t s);
/* call_index: batches bound before this one on the same d_history in this calibration run (0 for the first: the history's
 * two epoch accumulators alternate every 8 batches).  d_fallback may be NULL (see above). */
/* HOST: the compaction route's lists for just the pairs that need them.  h_states: a host copy of job.d_states (n_pairs + 1
 * entries) taken after dpl_octav_oneread_finish has run and the control block reported unfinished pairs (cnt_le != 0);
 * h_base_out [n_pairs + 1] receives whole-pair regions for those pairs (mode 1, not done), empty regions for the rest.  Returns
 * the elements ONE list takes: upload the table, allocate two lists of that many floats, point job.d_pair_base_full /
 * d_clist0 / d_clist1 at them and call dpl_octav_oneread_compaction (+ dpl_octav_finalize) — instead of binding the
 * whole-batch block of fallback_bytes. */
int64_t dpl_octav_fallback_layout(const dpl_octav_state* h_states, int64_t n_pairs, uint64_t* h_base_out);
int dpl_octav_plan_bind(const dpl_octav_plan* plan, void* d_tables, void* d_history, void* d_state, void* d_rescue, void* d_list0,
                        void* d_list1, void* d_fallback, const float* const* d_seg_ptrs, int64_t call_index, int dynamic_sym,
                        int max_iters, dpl_octav_oneread_job* job);
/* TEST HOOKS (0 = off; return the previous setting): _exact_ makes the exact walk of dpl_octav_run_bracket and the walk
 * of the exact-tail form reject every `every`-th pair, so that the restart paths — taken in production only when an iterate
 * leaves the gathered bins — can be exercised; _rescue_ does the same to the one-read form's rescue walk (-> compaction route). */
int dpl_test_hook_exact_fail_every(int every);
int dpl_test_hook_rescue_fail_every(int every);
/* d_out: fp32 [n_pairs,3] = (optimal_s, min, max) like the reference's per-image lists. */
int dpl_octav_finalize(const dpl_octav_state* d_states, int64_t n_pairs, float* d_out, dpl_stream_t s);

/* ---- per-output-channel weight ranges: replaces np.min/np.max(tensor.reshape(C,-1), -1)
 *      (basic_algorithm.py:88-90).  d_w row-major [rows, cols]. */
int dpl_rowwise_minmax(const float* d_w, int64_t rows, int64_t cols, float* d_min, float* d_max, dpl_stream_t s);

/* ---- per-channel statistics of a channels-last activation (--smooth): acc[c] = max(acc[c], max_r |x[r * cols + c]|), that is
 *      np.maximum(acc, np.abs(x).max(0)) for d_x row-major [rows, cols].  A RUNNING maximum: zero d_acc ([cols] fp32) once, then
 *      call batch after batch; d_acc must hold non-negative values or NaN.  Taken as an unsigned-integer maximum on the bits of
 *      |x| (integer atomics: the result does not depend on order): a NaN in a column or already in acc stays NaN (any NaN
 *      pattern), +-inf gives inf, -0.0 counts as +0.0.  16-byte loads when cols % 4 == 0 and d_x is 16-byte aligned, else a
 *      scalar kernel.  rows == 0: nothing is done; rows < 0, cols < 1, a null pointer with rows > 0: refused. */
int dpl_colwise_absmax(const float* d_x, int64_t rows, int64_t cols, float* d_acc, dpl_stream_t s);

/* ---- fused QuantizeLinear->DequantizeLinear (quantize.py:197-239; ONNX opset-13 semantics) and the
 *      reference-owned torch restatement quant_acti (weight_transform/ada_quant_layer.py:28-36):
 *      y = (clamp(rint(x / scale[c]) + zp[c], qlo, qhi) - zp[c]) * scale[c]
 *      n_channels == 1: per tensor.  Otherwise channel c = (i / inner) % n_channels. */
int dpl_fake_quant(const float* d_x, float* d_y, int64_t n, const float* d_scale, const int32_t* d_zp,
                   int64_t n_channels, int64_t inner, int32_t qlo, int32_t qhi, dpl_stream_t s);
/* The same pair with its producer's activation applied on the way in, so that a forward that does not expose the producer's output
 * moves 8 B per element for ReLU -> Q/DQ instead of 16 (the reference's merge-ReLU rule leaves a ReLU behind Conv / Gemm / Add
 * unquantised at its input, quantize.py:50-55, so its OUTPUT carries the Q/DQ pair of the next layer, :74-93):
 *   DPL_FQ_PRE_NONE      y = fq(x)                        (d_x2 ignored)
 *   DPL_FQ_PRE_RELU      y = fq(max(x, 0))                NaN stays NaN, as np.maximum / torch.relu
 *   DPL_FQ_PRE_ADD_RELU  y = fq(max(x + x2, 0))           one fp32 addition (round to nearest); d_x2: n floats, no broadcast */
#define DPL_FQ_PRE_NONE 0
#define DPL_FQ_PRE_RELU 1
#define DPL_FQ_PRE_ADD_RELU 2
int dpl_fake_quant_pre(int32_t pre, const float* d_x, const float* d_x2, float* d_y, int64_t n, const float* d_scale,
                       const int32_t* d_zp, int64_t n_channels, int64_t inner, int32_t qlo, int32_t qhi, dpl_stream_t s);
/* The same arithmetic over a WHOLE tensor set in one launch (a caller that holds every tensor of a forward: one launch instead
 * of one per Q/DQ pair — 123 for ResNet-50, most of them launch-bound): d_items / d_block_begin = a partition of the tensors'
 * elements (dpl_build_balanced_items over one span per tensor: item.seg = tensor, offset / count in elements; items are cut on
 * multiples of 1024 elements inside a tensor), d_seg_x / d_seg_y = the tensors' input / output base pointers (may be equal:
 * in place), d_params[tensor] = its quantisation parameters (all DEVICE memory). */
typedef struct dpl_fake_quant_params {
    const float* d_scale;          /* [n_channels] */
    const int32_t* d_zero_point;   /* [n_channels] */
    int64_t n_channels;            /* 1: per tensor */
    int64_t inner;                 /* elements per channel row: channel c = (i / inner) % n_channels */
    int32_t qlo, qhi;
} dpl_fake_quant_params;
int dpl_fake_quant_items(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin, int64_t n_blocks,
                         const float* const* d_seg_x, float* const* d_seg_y, const dpl_fake_quant_params* d_params, dpl_stream_t s);

/* ---- the same pair on the OCP FP8 E4M3 grid ("float8e4m3fn": bias 7, 3 mantissa bits, subnormal step 2^-9, largest finite
 *      value 448, no infinities) — ONNX opset 19 QuantizeLinear with a float8e4m3fn zero point and saturate = 1, followed by
 *      DequantizeLinear:
 *      y = fl32(e4m3_round(fl32(x / scale[c])) * scale[c])
 *      e4m3_round: the nearest e4m3fn value, round half to even (in the subnormal range too); |v| > 448 and +-inf give +-448;
 *      NaN stays NaN; the sign of zero is kept.  The division and the product are single fp32 operations.  No zero point, no
 *      qlo / qhi.  `pre`, d_x2, n_channels, inner: as dpl_fake_quant_pre. */
int dpl_fake_quant_fp8(int32_t pre, const float* d_x, const float* d_x2, float* d_y, int64_t n, const float* d_scale,
                       int64_t n_channels, int64_t inner, dpl_stream_t s);
/* ... over a whole tensor set in one launch: the arguments of dpl_fake_quant_items; d_zero_point, qlo and qhi of the parameter
 * rows are ignored (d_zero_point may be null). */
int dpl_fake_quant_fp8_items(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin, int64_t n_blocks,
                             const float* const* d_seg_x, float* const* d_seg_y, const dpl_fake_quant_params* d_params, dpl_stream_t s);

/* ---- the OCP Microscaling (MX) v1.0 Q/DQ pair (beyond the reference; --mx): the tensor is [outer, k, inner]; every 32
 *      consecutive indices along k, from 0, form a block (the last one holds the k % 32 elements that exist) with one shared
 *      scale 2^se, an E8M0 code, and elements of type `elem` — DPL_MX_E4M3 (MXFP8: OCP FP8 E4M3, emax 8, largest value 448) or
 *      DPL_MX_E2M1 (MXFP4: 0, 0.5, 1, 1.5, 2, 3, 4, 6; emax 2).  With a = max |v| of the block:
 *        a NaN or inf   every element of the block is NaN, scale code 0xFF
 *        a == 0         se = -127, the zeros keep their signs
 *        otherwise      se = max(floor(log2 a) - emax, -127)
 *      and y = round_elem(v / 2^se) * 2^se, round_elem: the nearest value of the format, ties to the even mantissa, saturating.
 *      Exact (bit operations: fp32 subnormal inputs and outputs are kept whatever the denormal mode); the definition is
 *      tests/mx_model.py.  d_scales_or_null: uint8 [outer, ceil(k / 32), inner], se + 127 per block.  d_y may equal d_x.
 *      1 <= k, inner < 2^31; outer * k * inner == 0 is a no-op. */
#define DPL_MX_E4M3 0
#define DPL_MX_E2M1 1
/* The two OCP MXFP6 formats (--mx mxfp6_e2m3 / mxfp6_e3m2; tests/mx_fp6_model.py is the definition).  Neither has NaN or inf codes.
 *      DPL_MX_E2M3  S.EE.MMM, bias 1: m / 8 under the exponent field 0, else (1 + m / 8) * 2^(field - 1); largest value 7.5, emax 2.
 *      DPL_MX_E3M2  S.EEE.MM, bias 3: m / 16 under the field 0, else (1 + m / 4) * 2^(field - 3); largest value 28, emax 4.
 * dpl_fake_quant_mx, dpl_fake_quant_mx_scaled, dpl_mx_scale_search, dpl_mx_encode, dpl_mx_encode_scaled, dpl_mx_decode, dpl_mx_gemm and
 * dpl_mx_conv take them; dpl_mx_gemm_err and dpl_gptq_mx_block are held to the first two.  Packed, a block's 32 codes are ONE little-endian
 * string of 192 bits, 24 bytes: code i occupies bits [6 i, 6 i + 6), i.e. byte (6 i) / 8 from bit (6 i) % 8 upward, carrying into the
 * next byte; codes [outer, inner, nblk * 24].  The codes' base must be 16-byte aligned as for the others (a block then lies at a
 * multiple of 8 bytes).  In a 0xFF block every code is 0.  The codes 2 .. 5 are not formats. */
#define DPL_MX_E2M3 6
#define DPL_MX_E3M2 7
int dpl_fake_quant_mx(int32_t elem, const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner,
                      uint8_t* d_scales_or_null, dpl_stream_t s);

/* ---- the element codes of an MX tensor and back (beyond the reference; --mx_pack; the definition is tests/mx_pack_model.py).
 *      dpl_mx_encode writes what dpl_fake_quant_mx computes, as bytes: with y its output and se / 0xFF its scale code per block,
 *        d_scales   the E8M0 byte, se + 127; 0xFF for a block that holds a NaN or an infinity
 *        E4M3       the OCP FP8 E4M3FN byte S.EEEE.MMM (bias 7) of y / 2^se, the sign bit of a zero kept; 0x7F for every element
 *                   that exists of a 0xFF block
 *        E2M1       four bits S.EE.M (bias 1; the magnitude is the index into 0, 0.5, 1, 1.5, 2, 3, 4, 6), two to a byte, the
 *                   element at the even index along k in the low nibble (ONNX FLOAT4E2M1); 0 in a 0xFF block
 *      LAYOUT: codes and scales are K-INNERMOST, the order a block-scaled GEMM reads both operands in.  With kp = 32 * ceil(k / 32):
 *        d_codes    uint8 [outer, inner, kp] (E4M3) or [outer, inner, kp / 2] (E2M1); elements past k of a short last block: code 0
 *        d_scales   uint8 [outer, inner, kp / 32]
 *      For inner > 1 this is a TRANSPOSE of the element order of the fp32 tensor [outer, k, inner], and the scales are NOT in the
 *      order of dpl_fake_quant_mx's d_scales_or_null ([outer, ceil(k / 32), inner]).
 *      dpl_mx_decode is defined on every byte pair: scale 0xFF -> NaN (0x7FC00000) for the whole block; E4M3 codes 0x7F and 0xFF
 *      -> NaN; otherwise +-value * 2^(scale - 127) exactly (at least 2^-136: an fp32 subnormal, kept whatever the denormal mode),
 *      +-inf above fp32's range (never a pair the encoder writes).  It writes the elements that exist, [outer, k, inner], and
 *      nothing past k.  dpl_mx_decode(dpl_mx_encode(x)) == dpl_fake_quant_mx(x) bit for bit.
 *      Limits and the no-op rule are dpl_fake_quant_mx's.  d_codes must be 16-byte aligned (refused otherwise: a block's 32 or 16
 *      bytes move as 16-byte vectors); d_x / d_y of any alignment (not 16-byte aligned, or k resp. inner % 4 != 0: element by
 *      element); d_scales must not be null. */
int dpl_mx_encode(int32_t elem, const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_codes, uint8_t* d_scales,
                  dpl_stream_t s);
int dpl_mx_decode(int32_t elem, const uint8_t* d_codes, const uint8_t* d_scales, uint64_t outer, uint64_t k, uint64_t inner, float* d_y,
                  dpl_stream_t s);

/* ---- error-minimising E8M0 scales for a constant MX operand (beyond the reference; --mx_scale_search; the definition is
 *      tests/mx_scale_model.py, nothing is held to a tolerance).  The tensor is [outer, k, inner], blocks of 32 along k as above.
 *      dpl_mx_scale_search: per block, with a = max |v| over the elements that exist,
 *        a NaN or inf   the byte is 0xFF, both errors are +inf
 *        a == 0         the byte is 0 (se = -127), both errors are 0
 *        otherwise      the candidates are se0 = max(floor(log2 a) - emax, -127), dpl_fake_quant_mx's, and se0 + 1; se0 + 1 is
 *                       dropped when it exceeds 127 - emax (the largest element times the scale must be an fp32 value).  Under a
 *                       candidate se: y = round_elem(v / 2^se) * 2^se, saturating; e[i] = (v[i] - y[i])^2 in fp64 (exact: the
 *                       difference is an fp32 value, its square an fp64 one); elements past k of a short last block are +0.0;
 *                       err = the fp64 sum of the 32 terms as a balanced tree in index order, e = e[0::2] + e[1::2] five times.
 *                       se0 + 1 is chosen iff err_1 < err_0: ties keep the floor.
 *        d_scales       uint8 [outer, ceil(k / 32), inner], the chosen se + 127 (the order of dpl_fake_quant_mx's d_scales_or_null)
 *        d_err_or_null  fp64 [outer, ceil(k / 32), inner, 2]: the error at the floor, the error at the chosen byte
 *      Exact whatever the fp32 denormal mode (every fp64 operand is built from bit patterns).  One read of d_x.
 *      dpl_fake_quant_mx_scaled / dpl_mx_encode_scaled: dpl_fake_quant_mx / dpl_mx_encode under GIVEN bytes, d_scales resp.
 *      d_scales_in in the [outer, ceil(k / 32), inner] order above.  A block that holds a NaN or an infinity is a 0xFF block
 *      whatever byte was given; a given byte of 0xFF, or one above 254 - emax, makes the block a 0xFF block too; every other block
 *      gets se = byte - 127 and the same rounding under it.  A 0xFF block has every element NaN, the packed scale byte 0xFF and the
 *      element codes 0x7F (E4M3) or 0 (E2M1).  d_scales_out is K-innermost, [outer, inner, kp / 32], like dpl_mx_encode's d_scales:
 *      the given bytes transposed, 0xFF where the block is a 0xFF block.
 *      dpl_mx_decode(dpl_mx_encode_scaled(x, s)) == dpl_fake_quant_mx_scaled(x, s) bit for bit, and with the bytes
 *      dpl_fake_quant_mx writes, dpl_fake_quant_mx_scaled(x, those) == dpl_fake_quant_mx(x).  d_y may equal d_x.
 *      Limits, the no-op rule, the null checks and the 16-byte rule for d_codes are those of the entry points they stand beside
 *      (d_scales, d_scales_in, d_scales_out must not be null); a refused call (-2) launches nothing. */
int dpl_mx_scale_search(int32_t elem, const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_scales,
                        double* d_err_or_null, dpl_stream_t s);
int dpl_fake_quant_mx_scaled(int32_t elem, const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner,
                             const uint8_t* d_scales, dpl_stream_t s);
int dpl_mx_encode_scaled(int32_t elem, const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, const uint8_t* d_scales_in,
                         uint8_t* d_codes, uint8_t* d_scales_out, dpl_stream_t s);

/* ---- the product of two packed MX operands on CDNA4's block-scaled matrix instruction, v_mfma_scale_f32_16x16x128_f8f6f4
 *      (beyond the reference; --mx_verify; the definition is tests/mx_gemm_model.py).  Both operands are K-INNERMOST, exactly what
 *      dpl_mx_encode writes — an "NT" product.  With kp = 32 * ceil(k / 32) and bits = 8 (E4M3) or 4 (E2M1) per operand:
 *        d_a_codes  uint8 [batch, m, kp * bits / 8]        d_a_scales  uint8 [batch, m, kp / 32]
 *        d_b_codes  uint8 [batch or 1, n, kp * bits / 8]   d_b_scales  uint8 [batch or 1, n, kp / 32]   (b_batched != 0: batch)
 *        d_c        fp32 [batch, m, n]:  C[b, i, j] = sum over kk < kp of a[b, i, kk] * b[b or 0, j, kk]
 *      a, b: the values dpl_mx_decode gives those bytes.  elem_a and elem_b are chosen independently (DPL_MX_E4M3 / DPL_MX_E2M1).
 *      The codes past k of a short last block TAKE PART in the sum: the encoder writes 0 there, and non-zero pad codes are summed.
 *      A [K, N] MatMul weight blocked along axis -2, or a Gemm weight with transB = 1 blocked along axis 1, is [N, kp] as packed.
 *      The sum is the instruction's own (measured on the MI355X): E2M1 x E2M1 products are added exactly up to the
 *      fp32 accumulation, |C - exact| <= kp * 2^-23 * S with S = sum |a| |b|; with an E4M3 operand the products of every run of 8
 *      consecutive k are first truncated to 2^-14 of the run's largest one, which can lose up to 7 * 2^-14 * S.
 *      NaN rule: C[b, i, j] is NaN if row i of A or row j of B holds a 0xFF scale byte or an E4M3 NaN code (0x7F, 0xFF) anywhere in
 *      its kp codes — the kernel sees to it whatever the instruction does with such bytes.  An all-zero block as the encoder writes
 *      it (scale byte 0, codes 0) contributes exactly 0 against finite data.
 *      d_a_codes and d_b_codes must be 16-byte aligned (refused otherwise).  1 <= m, n, k < 2^31; batch * m * n * k == 0 is a no-op;
 *      a refused call (-2) launches nothing. */
int dpl_mx_gemm(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                const uint8_t* d_b_scales, uint64_t batch, uint64_t m, uint64_t n, uint64_t k, int32_t b_batched, float* d_c, dpl_stream_t s);

/* ---- dpl_mx_gemm's product held against a reference without being written (beyond the reference; --mx_mixed measures a node in
 *      both element formats with it; the definition is tests/mx_mixed_model.py gemm_err_partials).  The operands, their layout, the
 *      grid (a workgroup per 64 x 64 tile of C) and the accumulators are dpl_mx_gemm's, bit for bit, its NaN rule included.
 *        d_ref           fp32 [batch, m, n]       d_bias_or_null  fp32 [n] or null
 *        d_part          fp64 [batch * tiles_m * tiles_n, 2], tiles_m = ceil(m / 64), tiles_n = ceil(n / 64), the row of tile
 *                        (tm, tn) of batch b being (b * tiles_m + tm) * tiles_n + tn
 *      Per element v of C inside the arrays: d = v - ref in fp32, with a bias (v + bias[col]) - ref as two fp32 operations;
 *      part[tile][0] = sum of (double)d * (double)d, part[tile][1] = sum of (double)ref * (double)ref, both squares exact.  Rows >= m
 *      and columns >= n contribute +0.0 and are not read from d_ref.  The order of the additions is part of the definition: with
 *      wave w owning rows 32 (w >> 1) .. and columns 32 (w & 1) .. of the tile, lane l adds its 16 terms one after the other over
 *      (i, reg, j) nested in that order, the term's row being 16 i + 4 (l >> 4) + reg and its column 16 j + (l & 15) of that
 *      quadrant; the 64 lane sums fold pairwise by xor-shuffles 1, 2, 4, 8, 16, 32 (as an array: e = e[0::2] + e[1::2], six
 *      times); the four wave sums are added as (w0 + w1) + (w2 + w3).  Every workgroup writes its own row of d_part with plain
 *      stores: no atomics, nothing to clear beforehand, the same bits on every run.
 *      Rules in their order: elem_a / elem_b; batch * m * n * k == 0 is a no-op that returns 0; null pointers (d_ref and d_part
 *      included, the bias may be null); 1 <= m, n, k < 2^31; "tensor too large"; d_a_codes and d_b_codes 16-byte aligned; the grid.
 *      A refused call (-2) launches nothing. */
int dpl_mx_gemm_err(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                    const uint8_t* d_b_scales, uint64_t batch, uint64_t m, uint64_t n, uint64_t k, int32_t b_batched, const float* d_ref,
                    const float* d_bias_or_null, double* d_part, dpl_stream_t s);

/* ---- a convolution of two packed MX operands on the same instruction, as an implicit GEMM (beyond the reference; --mx_conv; the
 *      definition is tests/mx_conv_model.py).  Both operands are what dpl_mx_encode writes along axis 1 (channels).  With
 *      cb = ceil(c / 32) and bb = 32 (E4M3) or 16 (E2M1) bytes per block of the operand's element format:
 *        d_a_codes  uint8 [n, h, w, cb * bb]          d_a_scales  uint8 [n, h, w, cb]          of an [n, c, h, w] activation (NHWC)
 *        d_b_codes  uint8 [cout, kh, kw, cb * bb]     d_b_scales  uint8 [cout, kh, kw, cb]     of a [cout, c, kh, kw] weight
 *        d_c        fp32 [n, oh, ow, cout] (NHWC):
 *          C[b, oy, ox, co] = sum over ky < kh, kx < kw, ch < 32 * cb of
 *                             a[b, oy * stride_h - pad_top + ky * dil_h, ox * stride_w - pad_left + kx * dil_w, ch] * b[co, ky, kx, ch]
 *      a, b: the values dpl_mx_decode gives those bytes; the pad codes of a short last channel block take part.  A tap outside the
 *      image contributes nothing and is never read, whatever oh and ow are: the caller computes them (and the pads at the bottom
 *      and on the right follow from them).  group = 1 only.  The sum is the instruction's own, over the kh * kw * cb K-blocks in the
 *      weight's memory order, four to a step: dpl_mx_gemm's error bound holds with kp = kh * kw * 32 * cb.
 *      NaN rule: C[b, oy, ox, co] is NaN if a block of A inside an in-image tap of that output, or any block of row co of B, holds a
 *      0xFF scale byte or an E4M3 NaN code (0x7F, 0xFF); a bad pixel that no tap of an output reaches leaves that output finite.
 *      The un-staged form: operands come straight from global memory, an activation block is read again for every tap.
 *      Refused (-2, nothing launched): an unknown element code; kh, kw, a stride or a dilation below 1; a negative pad; any argument
 *      negative or >= 2^31; null pointers; d_a_codes or d_b_codes not 16-byte aligned; kh * kw * cb or oh * ow >= 2^31, a tensor
 *      beyond 2^63 bytes or a grid beyond 2^31 workgroups.  n * h * w * c * cout * oh * ow == 0 is a no-op that returns 0. */
int dpl_mx_conv(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                const uint8_t* d_b_scales, int64_t n, int64_t h, int64_t w, int64_t c, int64_t cout, int64_t kh, int64_t kw, int64_t stride_h,
                int64_t stride_w, int64_t pad_top, int64_t pad_left, int64_t dil_h, int64_t dil_w, int64_t oh, int64_t ow, float* d_c,
                dpl_stream_t s);

/* ---- the block-Hadamard rotation of --mx_rotate (beyond the reference): y = x . blockdiag(H32) along the contiguous last axis of
 *      the [rows, k] tensor, H32[i][j] = (-1)^popcount(i & j) (Sylvester, natural order, symmetric, H32 . H32 = 32 I; NOT
 *      normalised: the constant operand of the product carries the 2^-5).  Per run of 32 consecutive elements, five stages h = 1, 2,
 *      4, 8, 16: for every i with (i & h) == 0, (v[i], v[i | h]) <- (v[i] + v[i | h], v[i] - v[i | h]), each a single fp32
 *      operation — bit-exact against tests/mx_rotate_model.py fwht32 (a NaN or an infinity anywhere in a block spreads over the
 *      whole block).  d_y may equal d_x.  k must be a multiple of 32 below 2^31; rows * k == 0 is a no-op. */
int dpl_hadamard32(const float* d_x, float* d_y, uint64_t rows, uint64_t k, dpl_stream_t s);

/* ---- GPTQ (Frantar et al., 2022; beyond the reference; --gptq): quantise nb consecutive columns of a weight matrix one after
 *      the other and push each column's rounding error onto the block's columns not yet rounded.  d_w: [rows, ldw] fp32 row-major,
 *      one output channel per row, updated IN PLACE in columns [c0, c0 + nb) only; d_u: [*, ldu] fp32 row-major, the upper Cholesky
 *      factor of the inverse Hessian (H^-1 = U^T U), read at rows and columns [c0, c0 + nb) only; d_err: [rows, nb] fp32.
 *      For j = 0 .. nb - 1, c = c0 + j, every operation a single fp32 operation (no FMA contraction), per row r:
 *        q = Q(w[r, c]);  e = (w[r, c] - q) / u[c, c];  w[r, c] = q;  err[r, j] = e;
 *        w[r, c0 + k] = w[r, c0 + k] - e * u[c, c0 + k]      for k = j + 1 .. nb - 1
 *      Q is the element quantiser of the Q/DQ pair above under scale[ch] (and zero_point[ch], qlo, qhi), ch = r when n_channels ==
 *      rows, 0 when n_channels == 1: fmt DPL_GRID_UNIFORM the integer grid of dpl_fake_quant (qlo < qhi), DPL_GRID_E4M3 the FP8 grid
 *      of dpl_fake_quant_fp8 (d_zero_point may be null; qlo, qhi ignored).  No reduction anywhere: the result is bit-exact against
 *      tests/gptq_model.py gptq_block whatever the launch geometry.  1 <= nb <= DPL_GPTQ_MAX_BLOCK, 0 <= c0, c0 + nb <= ldw and
 *      <= ldu; rows <= 0 is a no-op.  A refused call (-2) launches nothing. */
#define DPL_GPTQ_MAX_BLOCK 128
int dpl_gptq_block(float* d_w, int64_t rows, int64_t ldw, int64_t c0, int64_t nb, const float* d_u, int64_t ldu, const float* d_scale,
                   const int32_t* d_zero_point, int64_t n_channels, int32_t qlo, int32_t qhi, int32_t fmt, float* d_err, dpl_stream_t s);

/* ---- the same recursion on an MX block-scaled grid (--mx_gptq; elem: DPL_MX_E4M3 / DPL_MX_E2M1): d_w is [rows, ldw] with k <= ldw
 *      columns in use, MX blocks of 32 columns from column 0 (the last one holds the k % 32 that exist).  The grid of a block is fixed
 *      when the recursion ENTERS it: at every column c that is a multiple of 32, per row, a = max |w[r, c .. min(c + 32, k) - 1]| over
 *      the current values (the compensation of every earlier column included), se = the floor rule's shared exponent of
 *      dpl_fake_quant_mx (-127 for an all-zero block), d_scales[r * ld_scales + c / 32] = se + 127, and every column of the block is
 *      rounded as Q(v) = round_elem(v / 2^se) * 2^se, saturating at the largest element times 2^se — on bit patterns, whatever
 *      the code object's denormal mode.  DPL_MX_E4M3 only: a rounded magnitude of 1.875 * 2^t * 2^se that exceeds every magnitude the
 *      block has been given so far becomes the nearer of 1.75 * 2^t * 2^se (|v| not above it) and 2 * 2^t * 2^se — the format has no
 *      1.875 * 2^8, so such a value must not end up as the largest of a block that has shrunk below its entry binade.
 *      The rest is dpl_gptq_block's, operation for operation: bit-exact against
 *      tests/mx_gptq_model.py gptq_mx_block, d_err and the bytes included.  The finished block is a fixed point of
 *      dpl_fake_quant_mx.  A block whose entry maximum is a NaN or an infinity gets the byte 0xFF and NaN elements.
 *      Whole blocks only: c0 % 32 == 0, and nb % 32 == 0 unless c0 + nb == k; 1 <= nb <= DPL_GPTQ_MAX_BLOCK; c0 + nb <= k and <= ldu;
 *      ld_scales >= ceil(k / 32); rows below 2^31, rows <= 0 is a no-op.  A refused call (-2) launches nothing. */
int dpl_gptq_mx_block(int32_t elem, float* d_w, int64_t rows, int64_t ldw, int64_t k, int64_t c0, int64_t nb, const float* d_u, int64_t ldu,
                      float* d_err, uint8_t* d_scales, int64_t ld_scales, dpl_stream_t s);

/* ---- cosine-similarity partial sums (utils.py:273-278): d_acc[slot*3 + {0,1,2}] += sum(a*b), sum(a*a),
 *      sum(b*b) in fp64. */
int dpl_cos_accumulate(const float* d_a, const float* d_b, int64_t n, double* d_acc, int64_t slot, dpl_stream_t s);

/* Bias correction (bias_correction.py:9-13: bias += mean(fp_out - q_out) over every axis but the channel one):
 * a, b viewed as [outer, n_channels, inner] (Conv output [n, C, H, W]; Gemm output [n, C] with inner = 1);
 * d_acc[c] += sum over outer and inner of (a - b), accumulated in fp64. */
int dpl_channel_diff_sum(const float* d_a, const float* d_b, int64_t outer, int64_t n_channels, int64_t inner,
                         double* d_acc, dpl_stream_t s);

/* The classifier head of a convolutional network in the calibration forward (forward_net.py:192-237 runs the graph with
 * onnxruntime; here: MIOpen + this): C[m, n] = alpha * sum_k A[m, k] * B(k, n) + beta * bias(m, n), fp32, sums over k in ascending
 * order with one fused multiply-add per term.  A: [m, k] row-major; B(k, n) = d_b[k * b_stride_k + n * b_stride_n] (an ONNX Gemm with
 * transB = 1 passes (1, k)); bias(m, n) = d_bias[m * bias_stride_m + n * bias_stride_n] or no bias (NULL).  Products of at most
 * DPL_GEMM_SMALL_MAX multiply-adds only (csrc/gemm_small.hip says why this exists and what it is not). */
#define DPL_GEMM_SMALL_MAX (1ull << 28)
/* A product with few column tiles of C is cut along k (the partial sums are added in ascending order; the number of cuts depends on
 * n and k only, so a row of C is the same sum whatever m is): d_workspace = dpl_gemm_small_workspace(m, n, k) bytes of device memory (0: none needed, NULL is fine). */
uint64_t dpl_gemm_small_workspace(int64_t m, int64_t n, int64_t k);
int dpl_gemm_small(const float* d_a, const float* d_b, const float* d_bias, float* d_c, int64_t m, int64_t n, int64_t k,
                   int64_t b_stride_k, int64_t b_stride_n, int64_t bias_stride_m, int64_t bias_stride_n, float alpha, float beta,
                   float* d_workspace, dpl_stream_t s);

/* Same sums per work-item slot (slot = (image, tensor) pair in the profiling flow, profiling.py:57-64):
 * d_acc[slot*3 + {0,1,2}] += sum(a*b), sum(a*a), sum(b*b); a from d_seg_a, b from d_seg_b (same geometry). */
int dpl_cos_items_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                             int64_t n_blocks, const float* const* d_seg_a, const float* const* d_seg_b,
                             double* d_acc, dpl_stream_t s);

/* ------------------------------------------------------------------ AdaRound / BRECQ / QDrop inner loop (N4)
 * Replaces the eager torch arithmetic of weight_transform/ada_quant_layer.py:28-50 (quant_acti, quant_weight),
 * :96-112 (adaround_reg), :115-116 (L2_norm), :147 (round-mask initialisation) and the torch.optim.Adam update of
 * adaround.py:119-133 / brecq.py:158-186.  Weights are viewed as [n_channels, inner] (output channel first; a
 * ConvTranspose weight is transposed by the caller as adaround.py:58-59 does); scale / q_min / q_max hold
 * n_channels entries (1 for per-tensor).  `clamp` follows the reference: only its per-channel branch clamps
 * (the per-tensor branch discards the clamp result, ada_quant_layer.py:44-45). */
typedef struct dpl_round_step_params {
    double lr, adam_beta1, adam_beta2, adam_eps; /* torch.optim.Adam defaults: 1e-3, 0.9, 0.999, 1e-8 */
    int32_t step;      /* Adam step t >= 1 of this update */
    int32_t adam;      /* 0: gradients only (mask, moments and weight are left untouched) */
    int32_t clamp;
    int32_t reserved;
    float grad_scale;  /* multiplies dL/d(qw): 1 / world_size after a SUM all-reduce (DDP's mean), else 1 */
    float reg_beta;    /* regulariser temperature of this iteration (TempDecay, ada_quant_layer.py:119-134); 0: off */
    float reg_lambda;  /* regulariser weight (adaround_reg.alpha = 0.01) */
    float reserved2;
} dpl_round_step_params;

/* Device-resident schedule of a learner, so that a whole iteration can be captured in a hipGraph and replayed:
 * dpl_round_sched_advance (one thread) sets this iteration's regulariser temperature (TempDecay over t_max
 * iterations) and Adam bias corrections, then counts the iteration; dpl_round_step reads them when d_sched != NULL
 * (p->step, p->reg_beta are then ignored).  Zero-initialise before the first iteration. */
typedef struct dpl_round_sched {
    int32_t iter;       /* iterations completed */
    int32_t adam_step;  /* Adam steps completed */
    float reg_beta, step_size, bc2_sqrt, reserved;
} dpl_round_sched;
int dpl_round_sched_advance(dpl_round_sched* d_sched, int32_t t_max, double lr, double adam_beta1, double adam_beta2,
                            dpl_stream_t s);

/* wfloor = floor(w / scale);  alpha = -log((zeta - gamma) / (w / scale - wfloor - gamma) - 1)
 * n in [1, 2^32 - 2^20] (32-bit indices, grid stride up to 2^20), else -2: the same for the four calls below. */
int dpl_round_init(const float* d_w, const float* d_scale, int64_t n, int64_t n_channels, int64_t inner,
                   float* d_wfloor, float* d_alpha, dpl_stream_t s);
/* qw = clamp?(wfloor + h(alpha)) * scale;  h = rectified sigmoid (soft) or (alpha >= 0) (hard).
 * n in [1, 2^32 - 2^20]. */
int dpl_round_quant(const float* d_wfloor, const float* d_alpha, const float* d_scale, const float* d_qmin,
                    const float* d_qmax, int64_t n, int64_t n_channels, int64_t inner, int clamp, int soft,
                    float* d_qw, dpl_stream_t s);
/* One learning step in one pass: g = dL/d(alpha) from d_grad_qw (may be null) through the soft quantiser, plus
 * the regulariser's gradient; *d_reg_loss += lambda * sum(1 - |2h - 1|^beta) (may be null); Adam update of
 * alpha / m / v in place; d_qw_next (may be null) = the soft-quantised weight at the updated alpha;
 * d_grad_alpha (may be null) receives g.  n in [1, 2^32 - 2^20]. */
int dpl_round_step(const float* d_grad_qw, const float* d_wfloor, float* d_alpha, float* d_m, float* d_v,
                   const float* d_scale, const float* d_qmin, const float* d_qmax, int64_t n, int64_t n_channels,
                   int64_t inner, const dpl_round_step_params* p, const dpl_round_sched* d_sched, float* d_qw_next,
                   float* d_grad_alpha, double* d_reg_loss, dpl_stream_t s);
/* Sparse + quantised weight with a straight-through round (sparse_quant_layer.py:9-29, 61-66):
 * qw = clamp?(rint(w * mask / scale)) * scale; d_mask (0 / 1 per weight) may be null.  n in [1, 2^32 - 2^20]. */
int dpl_sparse_quant(const float* d_w, const float* d_mask, const float* d_scale, const float* d_qmin,
                     const float* d_qmax, int64_t n, int64_t n_channels, int64_t inner, int clamp, float* d_qw,
                     dpl_stream_t s);
/* Its gradient fused with torch.optim.SGD's update (sparse_quant.py:107-109: momentum, weight decay):
 * g = ((dL/dqw * grad_scale * scale) * clamp_pass) / scale * mask; d_grad_w (may be null) receives g; when `update`:
 * g += weight_decay * w; buf = first ? g : momentum * buf + g; w -= lr * buf (the two scaled adds fused, as
 * torch's add(alpha=) is).  n in [1, 2^32 - 2^20]. */
int dpl_sparse_step(const float* d_grad_qw, float* d_w, const float* d_mask, float* d_momentum_buf,
                    const float* d_scale, const float* d_qmin, const float* d_qmax, int64_t n, int64_t n_channels,
                    int64_t inner, int clamp, float grad_scale, float lr, float momentum, float weight_decay, int first,
                    int update, float* d_grad_w, dpl_stream_t s);
/* *d_loss += sum((y - target)^2) * inv_m with y = relu ? max(z, 0) : z  (L2_norm: inv_m = 1 / (elements / dim 1));
 * d_grad (may be null) = grad_coef * (y - target), zero where the ReLU is closed. */
int dpl_l2_loss(const float* d_z, const float* d_target, int64_t n, int relu, float grad_coef, double inv_m,
                float* d_grad, double* d_loss, dpl_stream_t s);
/* quant_acti with QDrop: y = rand < prob ? fake_quant(x) : x  (d_rand null: always quantised);
 * gradient as torch autograd defines it for the reference code: 0 through round(), 1 through the kept values. */
int dpl_acti_drop_fwd(const float* d_x, const float* d_rand, int64_t n, float scale, float qmin, float qmax,
                      float prob, float* d_y, dpl_stream_t s);
int dpl_acti_drop_bwd(const float* d_rand, const float* d_grad_y, int64_t n, float prob, float* d_grad_x,
                      dpl_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
