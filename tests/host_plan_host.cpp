// Host-side harness of csrc/host_plan.hpp (tests/test_host_plan_host.py): the HOST planning of the C ABI in a program of its own,
// built by the host compiler with the address and undefined-behaviour sanitizers.
//   host_plan_host in.u64 out.bin
// in:  u64 words.  n_cases, then per case: n_spans, n_tensors (0: no plan), n_blocks, chunk_elems, n_spans x (seg, offset, count, slot);
//      then n_states and n_states x (mode, done, n_elems) for dpl_octav_fallback_layout.
// out: records (u64 byte count, the bytes, padded to 8), in the order the code below writes them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../dipoorlet_amd/csrc/host_plan.hpp"

static FILE* g_out;
static void put(const void* p, uint64_t bytes) {
    static const char pad[8] = {0};
    fwrite(&bytes, 8, 1, g_out);
    if (bytes) fwrite(p, 1, bytes, g_out);
    fwrite(pad, 1, (8 - bytes % 8) % 8, g_out);
}
static void put_i64(int64_t v) { put(&v, 8); }
template <class T>
static void put_vec(const std::vector<T>& v) { put(v.data(), sizeof(T) * v.size()); }
static void put_err() { put(g_err, strlen(g_err)); }

static void one_case(const dpl_span* sp, int64_t n, int64_t n_tensors, int64_t n_blocks, uint64_t chunk) {
    {   // dpl_build_work_items: count (or the failure and its text), then the items
        const int64_t k = dpl_build_work_items(sp, n, chunk, nullptr, 0);
        put_i64(k);
        if (k < 0) put_err();
        std::vector<dpl_work_item> out((size_t)(k > 0 ? k : 0));
        if (k >= 0 && dpl_build_work_items(sp, n, chunk, out.data(), k) != k) abort();
        put_vec(out);
    }
    {   // dpl_build_balanced_items: count, items, block_begin
        const int64_t k = dpl_build_balanced_items(sp, n, n_blocks, nullptr, 0, nullptr);
        put_i64(k);
        std::vector<dpl_work_item> out((size_t)(k > 0 ? k : 0));
        std::vector<uint32_t> bb((size_t)(n_blocks + 1));
        if (dpl_build_balanced_items(sp, n, n_blocks, out.data(), k, bb.data()) != k) abort();
        put_vec(out);
        put_vec(bb);
    }
    {   // dpl_build_octav_slices: count (-3: refused, with its text), slices, pair_slice0
        const int64_t k = dpl_build_octav_slices(sp, n, nullptr, 0, nullptr);
        put_i64(k);
        if (k < 0) put_err();
        std::vector<dpl_work_item> out((size_t)(k > 0 ? k : 0));
        std::vector<uint32_t> ps((size_t)(2 * n));
        if (k >= 0 && dpl_build_octav_slices(sp, n, out.data(), k, ps.data()) != k) abort();
        put_vec(out);
        put_vec(ps);
    }
    if (n_tensors <= 0) return;
    dpl_octav_plan* p = dpl_octav_plan_create(sp, n, n_tensors, n_blocks);
    put_i64(p ? 1 : 0);
    if (!p) {
        put_err();
        return;
    }
    dpl_octav_workspace_sizes z;
    memset(&z, 0, sizeof(z));
    if (dpl_octav_plan_sizes(p, &z) != 0) abort();
    put(&z, sizeof(z));
    const uint64_t offs[9] = {p->off_slices, p->off_ps0, p->off_spans, p->off_base, p->off_basef, p->off_order, p->off_items, p->off_bb, p->tables};
    put(offs, sizeof(offs));
    put_vec(p->slices);
    put_vec(p->pair_slice0);
    put_vec(p->spans);
    put_vec(p->pair_base);
    put_vec(p->pair_base_full);
    put_vec(p->pair_order);
    put_vec(p->items);
    put_vec(p->block_begin);
    // jobs bound to fake addresses (never dereferenced), with and without a fallback block, over the epoch's call indices
    char* const base = (char*)(1ull << 40);
    for (const int64_t call : {0, 8, 9, 16})
        for (const int fb : {0, 1}) {
            dpl_octav_oneread_job j;
            if (dpl_octav_plan_bind(p, base, base + (1ull << 30), base + (2ull << 30), base + (3ull << 30), base + (4ull << 30), base + (5ull << 30),
                                    fb ? base + (7ull << 30) : nullptr, (const float* const*)(base + (6ull << 30)), call, (int)(call & 1), 20, &j) != 0)
                abort();
            put(&j, sizeof(j));
        }
    dpl_octav_plan_destroy(p);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    std::vector<uint64_t> in((size_t)ftell(f) / 8);
    fseek(f, 0, SEEK_SET);
    if (fread(in.data(), 8, in.size(), f) != in.size()) return 4;
    fclose(f);
    g_out = fopen(argv[2], "wb");
    if (!g_out) return 5;
    size_t at = 0;
    auto next = [&]() -> uint64_t {
        if (at >= in.size()) exit(6);
        return in[at++];
    };
    const uint64_t n_cases = next();
    for (uint64_t c = 0; c < n_cases; ++c) {
        const int64_t n = (int64_t)next(), n_tensors = (int64_t)next(), n_blocks = (int64_t)next();
        const uint64_t chunk = next();
        std::vector<dpl_span> sp((size_t)(n > 0 ? n : 1));   // (n_spans = 0 still passes a valid pointer)
        for (int64_t i = 0; i < n; ++i) {
            sp[i].seg = (uint32_t)next();
            sp[i].offset = next();
            sp[i].count = next();
            sp[i].slot = (uint32_t)next();
        }
        one_case(sp.data(), n, n_tensors, n_blocks, chunk);
    }
    const int64_t n_states = (int64_t)next();
    std::vector<dpl_octav_state> st((size_t)n_states + 1);   // (+ the control block behind the pairs' states)
    memset(st.data(), 0, sizeof(dpl_octav_state) * st.size());
    for (int64_t i = 0; i < n_states; ++i) {
        st[i].mode = (uint32_t)next();
        st[i].done = (uint32_t)next();
        st[i].n_elems = next();
    }
    std::vector<uint64_t> fb_base((size_t)n_states + 1, 99);
    put_i64(dpl_octav_fallback_layout(st.data(), n_states, fb_base.data()));
    put_vec(fb_base);
    put_i64(dpl_octav_fallback_layout(nullptr, n_states, fb_base.data()));
    put_err();
    fclose(g_out);
    return 0;
}
