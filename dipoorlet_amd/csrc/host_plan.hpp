// HOST planning of the C ABI: every table the streaming kernels index with is built here — pure index arithmetic, no HIP.
//   dpl_build_work_items / dpl_build_balanced_items   spans -> work items (fixed chunks / n_blocks balanced shares);
//   dpl_build_octav_slices                            pairs -> equal slices, largest pair first;
//   dpl_octav_plan_create / _destroy / _sizes / _bind the exact-tail form's tables, workspace sizes and job;
//   dpl_octav_fallback_layout                         the compaction route's list regions for the pairs a batch left over.
// A wrong entry in one of these tables is an out-of-range address in a kernel, so this code is kept where a plain C++
// compiler can build it: octav_tail_host.hip includes it for the library's definitions, tests/host_plan_host.cpp for a
// stand-alone program that runs it under the address and undefined-behaviour sanitizers (tests/test_host_plan_host.py).
// Exactly ONE translation unit of a program includes this header.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <stdexcept>
#include <vector>

#include "../../include/dipoorlet_hip.h"
#include "host_error.hpp"
#include "octav_geometry.hpp"

namespace {

inline dpl_work_item item_of(const dpl_span& sp, uint64_t offset, uint64_t count, uint32_t reserved) {
    return {offset, (uint32_t)count, sp.seg, sp.slot, reserved};
}

// a pair of n elements: c equal slices of `per` elements, cut on multiples of 4 (the last one takes the remainder)
struct SliceGeom {
    uint64_t c, per;
};
inline SliceGeom slice_geom(uint64_t n) {
    const uint64_t c = n == 0 ? 0 : (n + kSliceCap - 1) / kSliceCap;
    return {c, c == 0 ? 0 : (((n + c - 1) / c) + 3) & ~3ull};
}

// largest pairs first (the index breaks ties: a total order): the long ones start at once, the short ones fill the tail of
// the launch
inline std::vector<int64_t> largest_first(const dpl_span* spans, int64_t n_spans) {
    std::vector<int64_t> order((size_t)n_spans);
    for (int64_t i = 0; i < n_spans; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(),
              [spans](int64_t a, int64_t b) { return spans[a].count != spans[b].count ? spans[a].count > spans[b].count : a < b; });
    return order;
}

// slices of all pairs, or -3: a pair above kMaxCluster slices
inline int64_t count_slices(const dpl_span* spans, const std::vector<int64_t>& order) {
    int64_t n_total = 0;
    for (const int64_t i : order) {
        const uint64_t c = slice_geom(spans[i].count).c;
        if (c > kMaxCluster) {
            snprintf(g_err, sizeof(g_err), "dpl_build_octav_slices: a pair of %llu elements needs %llu slices (max %u)",
                     (unsigned long long)spans[i].count, (unsigned long long)c, kMaxCluster);
            return -3;
        }
        n_total += (int64_t)c;
    }
    return n_total;
}

// pair_slice0[2 slot], [2 slot + 1]: first and one-past-last slice of the pair in slot `slot` (slots 0 .. n_spans-1)
inline void fill_slices(const dpl_span* spans, const std::vector<int64_t>& order, dpl_work_item* out, uint32_t* pair_slice0) {
    const uint64_t n_spans = order.size();
    if (pair_slice0) std::fill(pair_slice0, pair_slice0 + 2 * n_spans, 0u);
    int64_t p = 0;
    for (const int64_t i : order) {
        const dpl_span& sp = spans[i];
        const SliceGeom g = slice_geom(sp.count);
        if (g.c == 0) continue;
        if (pair_slice0 && sp.slot < n_spans) {
            pair_slice0[2 * sp.slot] = (uint32_t)p;
            pair_slice0[2 * sp.slot + 1] = (uint32_t)(p + (int64_t)g.c);
        }
        uint64_t off = 0;
        for (uint64_t j = 0; j < g.c; ++j) {
            const uint64_t take = (j + 1 == g.c) ? sp.count - off : g.per;
            out[p++] = item_of(sp, sp.offset + off, take, (uint32_t)g.c);
            off += take;
        }
    }
}

inline uint64_t up256(uint64_t x) { return (x + 255ull) & ~255ull; }
template <class T>
inline uint64_t table_bytes(const std::vector<T>& v) { return up256(sizeof(T) * (uint64_t)(v.empty() ? 1 : v.size())); }

}  // namespace

// The exact-tail form as a SELF-SUFFICIENT ABI (forward_net.py:315-340 is the call site it serves): a HOST plan over the pairs of
// one tensor-set geometry knows every buffer's size, holds the static tables (dpl_octav_plan_upload copies them) and fills the
// job.  A caller allocates what dpl_octav_plan_sizes reports, nothing else.
struct dpl_octav_plan {
    int64_t n_pairs = 0, n_tensors = 0, n_slices = 0, n_multi = 0, n_small = 0, n_items = 0, n_blocks = 0, n_multi_slices = 0;
    uint64_t list_elems = 0, full_elems = 0;
    // host copies of the tables, in the order they sit in the device block (offsets below, bytes)
    std::vector<dpl_work_item> slices;
    std::vector<uint32_t> pair_slice0;
    std::vector<dpl_span> spans;
    std::vector<uint64_t> pair_base;        // [n_pairs + 1]: capped regions
    std::vector<uint64_t> pair_base_full;   // [n_pairs + 1]: whole-pair regions (the compaction route's lists)
    std::vector<uint32_t> pair_order;
    std::vector<dpl_work_item> items;
    std::vector<uint32_t> block_begin;
    uint64_t off_slices = 0, off_ps0 = 0, off_spans = 0, off_base = 0, off_basef = 0, off_order = 0, off_items = 0, off_bb = 0, tables = 0;
};

namespace {

// the layout of the per-batch blocks (bytes from their base)
inline uint64_t state_pred_off(const dpl_octav_plan* p) { return up256(sizeof(dpl_octav_state) * (uint64_t)(p->n_pairs + 1)); }
inline uint64_t rescue_missed_off(const dpl_octav_plan* p) { return up256(sizeof(uint32_t) * (uint64_t)kLogWords * (uint64_t)p->n_pairs); }
inline uint64_t rescue_resc_off(const dpl_octav_plan* p) { return rescue_missed_off(p) + up256(sizeof(uint32_t) * 3ull * (uint64_t)p->n_pairs); }
inline uint64_t rescue_lh_off(const dpl_octav_plan* p) { return rescue_resc_off(p) + up256(8ull * (uint64_t)kRescRow * (uint64_t)p->n_pairs); }

}  // namespace

extern "C" {

int64_t dpl_build_work_items(const dpl_span* spans, int64_t n_spans, uint64_t chunk_elems, dpl_work_item* out,
                             int64_t cap) {
    if (!spans || n_spans < 0 || chunk_elems == 0 || (chunk_elems % 1024) != 0 || chunk_elems > 0xFFFFFC00ull)
        return fail_msg("dpl_build_work_items: chunk_elems must be a non-zero multiple of 1024 below 2^32");
    int64_t n = 0;
    for (int64_t i = 0; i < n_spans; ++i) {
        uint64_t off = spans[i].offset, left = spans[i].count;
        while (left) {
            const uint64_t c = left < chunk_elems ? left : chunk_elems;
            if (out && n < cap) out[n] = item_of(spans[i], off, c, 0);
            ++n;
            off += c;
            left -= c;
        }
    }
    return n;
}

int64_t dpl_build_balanced_items(const dpl_span* spans, int64_t n_spans, int64_t n_blocks, dpl_work_item* out,
                                 int64_t cap, uint32_t* block_begin) {
    if (!spans || n_spans < 0 || n_blocks < 1) return fail_msg("dpl_build_balanced_items: bad arguments");
    unsigned __int128 total = 0;
    for (int64_t i = 0; i < n_spans; ++i) total += spans[i].count;
    int64_t n = 0;
    int64_t si = 0;
    uint64_t lo = 0;       // offset inside span si
    unsigned __int128 g = 0;  // global position of the cursor in the concatenated element stream
    for (int64_t b = 0; b < n_blocks; ++b) {
        if (block_begin) block_begin[b] = (uint32_t)n;
        const unsigned __int128 target = (b + 1 == n_blocks) ? total : (total * (unsigned __int128)(b + 1)) / (unsigned __int128)n_blocks;
        while (si < n_spans && g < target) {
            const uint64_t remaining = spans[si].count - lo;
            if (remaining == 0) {
                ++si;
                lo = 0;
                continue;
            }
            const unsigned __int128 want = target - g;
            const bool span_done = want >= remaining;
            const uint64_t take = span_done ? remaining : ((uint64_t)want / 1024u) * 1024u;  // cut points stay 4 KiB-aligned inside a span
            if (take == 0) break;  // less than one aligned piece left for this block: next block takes it
            uint64_t off = spans[si].offset + lo, left = take;
            while (left) {  // a share larger than 2^32-1024 elements is emitted as several items
                const uint64_t c = left < 0xFFFFFC00ull ? left : 0xFFFFFC00ull;
                if (out && n < cap) out[n] = item_of(spans[si], off, c, 0);
                ++n;
                off += c;
                left -= c;
            }
            g += take;
            lo += take;
            if (!span_done) break;
            ++si;
            lo = 0;
        }
    }
    if (block_begin) block_begin[n_blocks] = (uint32_t)n;
    return n;
}

uint32_t dpl_octav_slice_cap(void) { return kSliceCap; }
uint32_t dpl_octav_list_cap(uint64_t n_elements) { return list_cap_of(n_elements); }
uint32_t dpl_octav_small_pair(void) { return kSmallCap; }

int64_t dpl_build_octav_slices(const dpl_span* spans, int64_t n_spans, dpl_work_item* out, int64_t cap, uint32_t* pair_slice0) {
    if (!spans || n_spans < 0) return fail_msg("dpl_build_octav_slices: bad arguments");
    try {
        const std::vector<int64_t> order = largest_first(spans, n_spans);
        const int64_t n_total = count_slices(spans, order);
        if (n_total >= 0 && out && n_total <= cap) fill_slices(spans, order, out, pair_slice0);
        return n_total;
    } catch (const std::bad_alloc&) {
        return fail_msg("dpl_build_octav_slices: out of memory");
    } catch (const std::length_error&) {
        return fail_msg("dpl_build_octav_slices: too many spans");
    }
}

dpl_octav_plan* dpl_octav_plan_create(const dpl_span* spans, int64_t n_spans, int64_t n_tensors, int64_t n_blocks) {
    if (!spans || n_spans < 1 || n_tensors < 1 || n_blocks < 1) {
        fail_msg("dpl_octav_plan_create: bad arguments");
        return nullptr;
    }
    for (int64_t i = 0; i < n_spans; ++i)
        if (spans[i].slot != (uint32_t)i) {
            fail_msg("dpl_octav_plan_create: spans must carry slots 0 .. n_spans-1 in order (slot = image * n_tensors + tensor)");
            return nullptr;
        }
    dpl_octav_plan* p = nullptr;
    try {
        // pair order: largest first — the multi-slice pairs are its first n_multi entries, the small pairs its last n_small
        const std::vector<int64_t> order = largest_first(spans, n_spans);
        const int64_t ns = count_slices(spans, order);
        if (ns < 0) return nullptr;   // (-3: a pair above 64 slices: dpl_octav_run_bracket serves such a set)
        p = new dpl_octav_plan();
        p->n_pairs = n_spans;
        p->n_tensors = n_tensors;
        p->n_blocks = n_blocks;
        p->n_slices = ns;
        p->slices.resize((size_t)ns);
        p->pair_slice0.resize((size_t)(2 * n_spans));
        fill_slices(spans, order, p->slices.data(), p->pair_slice0.data());
        p->spans.assign(spans, spans + n_spans);
        p->pair_order.assign(order.begin(), order.end());
        // list regions, in pair order: a single-slice pair list_cap_of(n) values, a pair of c slices c parts of list_cap_of(slice)
        p->pair_base.assign((size_t)(n_spans + 1), 0);
        p->pair_base_full.assign((size_t)(n_spans + 1), 0);
        for (int64_t i = 0; i < n_spans; ++i) {
            const uint64_t n = spans[i].count;
            const SliceGeom g = slice_geom(n);
            const uint64_t region = g.c == 1 ? list_cap_of(n) : g.c * (uint64_t)list_cap_of(g.per);
            p->pair_base[i + 1] = p->pair_base[i] + region;
            p->pair_base_full[i + 1] = p->pair_base_full[i] + ((n + 31ull) & ~31ull);
            if (g.c > 1) p->n_multi += 1, p->n_multi_slices += (int64_t)g.c;
            if (n <= kSmallCap) p->n_small += 1;
        }
        p->list_elems = p->pair_base[n_spans];
        p->full_elems = p->pair_base_full[n_spans];
        // the balanced partition of the same pairs (the compaction route's kernels)
        const int64_t ni = dpl_build_balanced_items(spans, n_spans, n_blocks, nullptr, 0, nullptr);
        p->n_items = ni;
        p->items.resize((size_t)ni);
        p->block_begin.resize((size_t)(n_blocks + 1));
        dpl_build_balanced_items(spans, n_spans, n_blocks, p->items.data(), ni, p->block_begin.data());
        uint64_t o = 0;
        p->off_slices = o, o += table_bytes(p->slices);
        p->off_ps0 = o, o += table_bytes(p->pair_slice0);
        p->off_spans = o, o += table_bytes(p->spans);
        p->off_base = o, o += table_bytes(p->pair_base);
        p->off_basef = o, o += table_bytes(p->pair_base_full);
        p->off_order = o, o += table_bytes(p->pair_order);
        p->off_items = o, o += table_bytes(p->items);
        p->off_bb = o, o += table_bytes(p->block_begin);
        p->tables = o;
        return p;
    } catch (const std::bad_alloc&) {
        fail_msg("dpl_octav_plan_create: out of memory");
    } catch (const std::length_error&) {
        fail_msg("dpl_octav_plan_create: too many spans or blocks");
    }
    delete p;   // (only an allocation failure comes here)
    return nullptr;
}

void dpl_octav_plan_destroy(dpl_octav_plan* p) { delete p; }

int dpl_octav_plan_sizes(const dpl_octav_plan* p, dpl_octav_workspace_sizes* out) {
    if (!p || !out) return fail_msg("dpl_octav_plan_sizes: null argument");
    out->tables_bytes = p->tables;
    out->history_bytes = sizeof(uint32_t) * 2ull * (uint64_t)p->n_tensors * (uint64_t)kLogWords;
    out->state_bytes = state_pred_off(p) + up256(sizeof(uint32_t) * (uint64_t)kPredRow * (uint64_t)p->n_tensors);
    out->rescue_bytes = rescue_lh_off(p) + 8ull * (uint64_t)kLogNB * (uint64_t)p->n_multi_slices;
    out->list_bytes = 4ull * (p->list_elems > 0 ? p->list_elems : 32ull);
    out->fallback_bytes = 2ull * 4ull * (p->full_elems > 0 ? p->full_elems : 32ull);
    out->result_bytes = sizeof(float) * 3ull * (uint64_t)p->n_pairs;
    out->n_pairs = p->n_pairs;
    out->n_slices = p->n_slices;
    out->n_multi = p->n_multi;
    out->n_small = p->n_small;
    return 0;
}

int dpl_octav_plan_bind(const dpl_octav_plan* p, void* d_tables, void* d_history, void* d_state, void* d_rescue, void* d_list0,
                        void* d_list1, void* d_fallback, const float* const* d_seg_ptrs, int64_t call_index, int dynamic_sym,
                        int max_iters, dpl_octav_oneread_job* j) {
    if (!p || !j || !d_tables || !d_history || !d_state || !d_rescue || !d_list0 || !d_list1)
        return fail_msg("dpl_octav_plan_bind: null argument");
    if (call_index < 0) return fail_msg("dpl_octav_plan_bind: negative call index");
    memset(j, 0, sizeof(*j));
    char* t = (char*)d_tables;
    j->d_slices = (const dpl_work_item*)(t + p->off_slices);
    j->n_slices = p->n_slices;
    j->d_pair_slice0 = (const uint32_t*)(t + p->off_ps0);
    j->d_pair_spans = (const dpl_span*)(t + p->off_spans);
    j->d_pair_base = (const uint64_t*)(t + p->off_base);
    j->d_pair_base_full = (const uint64_t*)(t + p->off_basef);
    j->d_pair_order = (const uint32_t*)(t + p->off_order);
    j->n_pairs = p->n_pairs;
    j->n_tensors = p->n_tensors;
    j->n_small = p->n_small;
    j->n_multi = p->n_multi;
    j->d_items = (const dpl_work_item*)(t + p->off_items);
    j->n_items = p->n_items;
    j->d_block_begin = (const uint32_t*)(t + p->off_bb);
    j->n_blocks = p->n_blocks;
    j->d_seg_ptrs = d_seg_ptrs;
    j->d_states = (dpl_octav_state*)d_state;
    j->d_pred = (uint32_t*)((char*)d_state + state_pred_off(p));
    char* r = (char*)d_rescue;
    j->d_rescue_bm = (uint32_t*)r;
    j->d_missed = (uint32_t*)(r + rescue_missed_off(p));
    j->d_resc = (uint64_t*)(r + rescue_resc_off(p));
    j->d_lh = (uint64_t*)(r + rescue_lh_off(p));
    j->d_list0 = (float*)d_list0;
    j->d_list1 = (float*)d_list1;
    if (d_fallback) {
        j->d_clist0 = (float*)d_fallback;
        j->d_clist1 = (float*)d_fallback + (p->full_elems > 0 ? p->full_elems : 32ull);
    }
    j->d_vis = (uint32_t*)d_history;
    // two alternating epoch accumulators of kPlanEpoch batches each: batch k adds to accumulator (k / epoch) % 2, cleared by the
    // first batch of an epoch (dpl_octav_oneread_prepare)
    j->write_epoch = (int32_t)((call_index / kPlanEpoch) % 2);
    j->reset_epoch = (call_index % kPlanEpoch) == 0 ? 1 : 0;
    j->dynamic_sym = dynamic_sym;
    j->max_iters = max_iters;
    j->compaction_inline = d_fallback ? 1 : 0;
    return 0;
}

// HOST: where the compaction route's lists hold the pairs that are still unfinished after dpl_octav_oneread_finish — whole-pair
// regions for those pairs (mode 1, not done), empty ones for every other pair: a caller that reads the states back when the
// control block reports such pairs allocates two lists of the returned size instead of two whole-batch ones (14 pairs of a cold
// ResNet-50 batch of 3 936: 40 MB instead of 6.8 GB).
int64_t dpl_octav_fallback_layout(const dpl_octav_state* h_states, int64_t n_pairs, uint64_t* h_base_out) {
    if (!h_states || !h_base_out || n_pairs < 0) return fail_msg("dpl_octav_fallback_layout: bad arguments");
    uint64_t at = 0;
    for (int64_t i = 0; i < n_pairs; ++i) {
        h_base_out[i] = at;
        if (h_states[i].mode == 1u && !h_states[i].done) at += (h_states[i].n_elems + 31ull) & ~31ull;
    }
    h_base_out[n_pairs] = at;
    return (int64_t)at;
}

}  // extern "C"
