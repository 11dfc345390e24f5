// OCTAV ('-A mse', forward_net.py:284-342) in ONE read of the activations: the HOST side of the exact-tail form — the C ABI that
// launches it, and the definitions of the C ABI's host planning.
//
// Why not two reads: measured on MI355X (scripts/mall_probe.hip, profiles/r02/mall_probe.txt) a re-read of recently
// streamed data costs the same whether HBM or the 256 MiB Infinity Cache serves it (6.1-6.9 TB/s either way, one
// shared fabric), so the two-read bracket form of octav_kernels.hip cannot pass ~40 % of the roofline.  And a form that
// keeps a pair on chip until a leader has walked its bracket (tried first, round 2) spends its time waiting.
//
// Where everything is:
//   octav_wave.hpp     the workgroup's shape and static LDS block (Shared), the wave64 scans and sums by DPP, the suffix totals, the
//                        row loader of a list, the row of a rescued pair;
//   octav_tail.hpp     k_octav_tail / k_octav_tail_merge / k_octav_tail_init: one workgroup per slice streams it (min / max, exact
//                        log-scale histogram in LDS, the values at or above a threshold bin listed) and walks the pair — early
//                        iterates as lower bounds from the histogram, late ones exactly from the list; TailLds: their dynamic LDS;
//   octav_rescue.hpp   walk_rescued + k_octav_walk_rescue: the RESCUE of a pair whose walk was refused — the reference's whole
//                        iterate sequence on (exact totals of the bins above) + (the values of the pair's exact bracket, re-read
//                        by k_octav_rescue_gather in octav_kernels.hip), every iterate verified;
//   this file          check_job, dpl_octav_oneread_* and dpl_octav_plan_upload: one job struct per batch, launched and uploaded
//                        from here;
//   host_plan.hpp      the HOST planning of the whole C ABI — the work-item builders, the slices, the plan that sizes, lays out
//                        and binds a job — which has no HIP in it: this translation unit holds its definitions.
// Rounds 2 - 3 listed the bins ALL iterates were predicted to visit (k_octav_oneread, k_octav_probe, k_octav_sort,
// k_octav_walk[_sorted]: DESIGN 3c, 3d); the exact-tail form superseded them in round 4 and round 5 removed them.
// No workgroup ever waits for another; what crosses kernels crosses launches.
#include "common.hpp"
#include "octav_common.hpp"
#include "octav_wave.hpp"
#include "octav_tail.hpp"
#include "octav_rescue.hpp"
#include "host_plan.hpp"   // the HOST planning of the C ABI: definitions, for the whole library

#pragma clang fp contract(off)

extern "C" {

static int check_job(const char* who, const dpl_octav_oneread_job* j) {
    if (!j) return fail_msg("dpl_octav_oneread: null job");
    if (j->n_pairs <= 0 || j->n_slices <= 0) return 1;   // nothing to do
    if (j->n_tensors < 1 || (j->write_epoch != 0 && j->write_epoch != 1)) {
        snprintf(g_err, sizeof(g_err), "%s: bad tensor count / epoch", who);
        return -1;
    }
    if (!j->d_slices || !j->d_pair_slice0 || !j->d_pair_spans || !j->d_pair_base || !j->d_pair_order || !j->d_seg_ptrs ||
        !j->d_states || !j->d_pred || !j->d_list0 || !j->d_list1 || !j->d_rescue_bm || !j->d_missed || !j->d_vis || !j->d_resc ||
        (j->n_multi > 0 && !j->d_lh)) {
        snprintf(g_err, sizeof(g_err), "%s: null buffer in the job", who);
        return -1;
    }
    if (j->n_small < 0 || j->n_small > j->n_pairs || j->n_multi < 0 || j->n_multi > j->n_pairs) {
        snprintf(g_err, sizeof(g_err), "%s: bad small-pair / multi-slice-pair count", who);
        return -1;
    }
    return 0;
}
#define DPL_JOB_CHECK(who)                       \
    if (int e_ = check_job(who, j)) return e_ > 0 ? 0 : e_

// state of every pair + the control block, and the tensors' threshold snapshot (what their pairs asked for in the current and
// the previous epoch of batches)
int dpl_octav_oneread_prepare(const dpl_octav_oneread_job* j, dpl_stream_t s) {
    DPL_JOB_CHECK("dpl_octav_oneread_prepare");
    const int64_t vis_words = j->n_tensors * kLogWords;
    uint32_t* d_vis_w = j->d_vis + (int64_t)j->write_epoch * vis_words;
    const uint32_t* d_vis_o = j->d_vis + (int64_t)(1 - j->write_epoch) * vis_words;
    const int64_t n = j->n_pairs + 1 > j->n_tensors ? j->n_pairs + 1 : j->n_tensors;
    hipLaunchKernelGGL(k_octav_tail_init, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, j->d_states, j->n_pairs, d_vis_w, d_vis_o,
                       j->d_pred, j->n_tensors, j->reset_epoch);
    DPL_LAUNCH_CHECK("k_octav_tail_init");
    return 0;
}

// the batch's only read of the activations: k_octav_tail streams AND walks every single-slice pair; the slices of a pair above one
// slice leave their rows for k_octav_tail_merge
int dpl_octav_oneread_stream(const dpl_octav_oneread_job* j, dpl_stream_t s) {
    DPL_JOB_CHECK("dpl_octav_oneread_stream");
    const TailArgs fa{j->d_vis + (int64_t)j->write_epoch * j->n_tensors * kLogWords, j->d_pred, j->d_rescue_bm, j->d_missed,
                      reinterpret_cast<unsigned long long*>(j->d_resc), j->dynamic_sym, j->max_iters, g_exact_fail_every};
    const size_t lds = TailLds::bytes();
    // (a slice of a pair above one slice — the first items of d_slices, largest first — leaves its row in d_lh ...)
    hipLaunchKernelGGL(k_octav_tail, dim3((unsigned)j->n_slices), dim3(kThreads), lds, (hipStream_t)s, j->d_slices,
                       j->d_seg_ptrs, j->d_states, (uint32_t)j->n_tensors, j->d_pair_base, j->d_list0, j->d_states + j->n_pairs,
                       j->d_pair_spans, reinterpret_cast<unsigned long long*>(j->d_lh), fa);
    DPL_LAUNCH_CHECK("k_octav_tail");
    if (j->n_multi > 0) {   // ... which one workgroup per such pair adds up and walks (d_pair_order: these pairs come first)
        hipLaunchKernelGGL(k_octav_tail_merge, dim3((unsigned)j->n_multi), dim3(kThreads), lds, (hipStream_t)s, j->d_slices, j->d_states,
                           (uint32_t)j->n_tensors, j->d_pair_base, j->d_list0, j->d_states + j->n_pairs, j->d_pair_spans,
                           reinterpret_cast<const unsigned long long*>(j->d_lh), j->d_pair_order, j->d_pair_slice0, fa);
        DPL_LAUNCH_CHECK("k_octav_tail_merge");
    }
    return 0;
}

// Everything behind the streaming kernel, in stream order, nothing decided on the host: the RESCUE of the pairs whose walk was
// refused (k_octav_rescue_gather: those pairs re-read alone for their exact bracket's bins; k_octav_walk_rescue: the verified walk
// of every iterate), then — compaction_inline — the compaction route for what even that could not finish.  Both kernels return
// at once when the control block lists nothing (the usual case: 3 of 3 936 pairs of a ResNet-50 batch are rescued).
int dpl_octav_oneread_finish(const dpl_octav_oneread_job* j, dpl_stream_t s) {
    DPL_JOB_CHECK("dpl_octav_oneread_finish");
    hipStream_t st = (hipStream_t)s;
    dpl_octav_state* ctl = j->d_states + j->n_pairs;
    if (j->max_iters <= 0) return 0;
    if (int e = dpl_octav_rescue_gather_launch(j->d_missed, j->d_states, j->n_pairs, j->d_pair_spans, j->d_seg_ptrs, j->d_rescue_bm,
                                               j->d_pair_base, j->d_list1, st))
        return e;
    hipLaunchKernelGGL(k_octav_walk_rescue, dim3(kRescueGrid), dim3(kThreads), 0, st, j->d_states, ctl, j->d_pair_base, j->max_iters,
                       g_rescue_fail_every, j->d_rescue_bm, j->d_missed, j->d_list1, reinterpret_cast<const unsigned long long*>(j->d_resc));
    DPL_LAUNCH_CHECK("k_octav_walk_rescue");
    return j->compaction_inline ? dpl_octav_oneread_compaction(j, s) : 0;
}

// The compaction route for the pairs the control block counts in cnt_le (after dpl_octav_oneread_finish): what neither the walk
// nor the rescue could finish.  Its kernels return at once when there is none, but a caller that can read the count later (the
// pipeline: two batches on) skips the call — four launches with large footprints would otherwise wait for slots beside the
// next batch's streaming kernel.
int dpl_octav_oneread_compaction(const dpl_octav_oneread_job* j, dpl_stream_t s) {
    DPL_JOB_CHECK("dpl_octav_oneread_compaction");
    if (j->max_iters <= 0) return 0;
    if (int e = check_blocks("dpl_octav_oneread_compaction", j->n_items, j->d_block_begin, j->n_blocks)) return e;
    hipStream_t st = (hipStream_t)s;
    // its own whole-pair list regions (d_pair_base_full) in its own two lists: the one-read forms' lists hold list_cap_of(n)
    // values per pair, and the streaming kernel of a later batch may be writing d_list0 by now
    if (!j->d_pair_base_full || !j->d_clist0 || !j->d_clist1)
        return fail_msg("dpl_octav_oneread_compaction: the compaction route's lists (d_pair_base_full, d_clist0, d_clist1) are missing");
    return dpl_octav_fallback_route(j->d_items, j->n_items, j->d_block_begin, j->n_blocks, j->d_seg_ptrs, j->d_states, j->n_pairs,
                                    j->d_pair_spans, j->d_pair_base_full, j->d_pair_order, j->d_clist0, j->d_clist1, j->dynamic_sym,
                                    j->max_iters, st);
}

// The one plan function that calls the HIP runtime (the others, and struct dpl_octav_plan, are in host_plan.hpp)
int dpl_octav_plan_upload(const dpl_octav_plan* p, void* d_tables, dpl_stream_t s) {
    if (!p || !d_tables) return fail_msg("dpl_octav_plan_upload: null argument");
    char* d = (char*)d_tables;
    hipStream_t st = (hipStream_t)s;
    const struct { uint64_t off; const void* src; uint64_t bytes; } parts[] = {
        {p->off_slices, p->slices.data(), sizeof(dpl_work_item) * (uint64_t)p->n_slices},
        {p->off_ps0, p->pair_slice0.data(), sizeof(uint32_t) * 2ull * (uint64_t)p->n_pairs},
        {p->off_spans, p->spans.data(), sizeof(dpl_span) * (uint64_t)p->n_pairs},
        {p->off_base, p->pair_base.data(), sizeof(uint64_t) * (uint64_t)(p->n_pairs + 1)},
        {p->off_basef, p->pair_base_full.data(), sizeof(uint64_t) * (uint64_t)(p->n_pairs + 1)},
        {p->off_order, p->pair_order.data(), sizeof(uint32_t) * (uint64_t)p->n_pairs},
        {p->off_items, p->items.data(), sizeof(dpl_work_item) * (uint64_t)p->n_items},
        {p->off_bb, p->block_begin.data(), sizeof(uint32_t) * (uint64_t)(p->n_blocks + 1)},
    };
    for (const auto& q : parts) {
        if (q.bytes == 0) continue;
        const hipError_t e = hipMemcpyAsync(d + q.off, q.src, q.bytes, hipMemcpyHostToDevice, st);   // (the plan owns the sources)
        if (e != hipSuccess) return fail("dpl_octav_plan_upload", e);
    }
    return 0;
}

int dpl_octav_run_oneread(const dpl_octav_oneread_job* j, dpl_stream_t s) {
    if (int e = dpl_octav_oneread_prepare(j, s)) return e;
    if (int e = dpl_octav_oneread_stream(j, s)) return e;
    if (int e = dpl_octav_oneread_finish(j, s)) return e;
    return j && !j->compaction_inline ? dpl_octav_oneread_compaction(j, s) : 0;
}

}  // extern "C"
