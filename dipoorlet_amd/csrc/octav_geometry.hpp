// The numbers the OCTAV kernels (octav_common.hpp, octav_wave.hpp, octav_tail.hpp, octav_rescue.hpp), their launchers
// (octav_kernels.hip, octav_tail_host.hip) and the host planning of their tables (host_plan.hpp) must agree on: one definition each.  Plain constexpr, no HIP: usable from device code, from the library's
// host code and from a program a plain C++ compiler builds.
#pragma once
#include <stdint.h>

namespace {

constexpr int kLogNB = 2048;                       // bins of the log-scale histogram (octav_common.hpp has its geometry)
constexpr int kLogWords = kLogNB / 32;             // u32 words of a bitmap over them

constexpr uint32_t kSliceCap = 1044480;            // elements of a slice (streamed tile by tile)
static_assert(kSliceCap < (1u << 20) && kSliceCap % 4096u == 0u, "a slice's bin counts must fit the packed field");
constexpr uint32_t kMaxCluster = 64;               // slices of one pair at most
// pairs this small list their whole window (every step of their walk is exact): their list region holds all of them (list_cap_of)
constexpr uint32_t kSmallCap = 20480;
constexpr int64_t kPlanEpoch = 8;                  // batches per threshold-history epoch (dpl_octav_plan_bind)
constexpr int kPredRow = 2 * kLogWords;            // u32 words of a tensor's row in d_pred (word 0: the threshold snapshot)
constexpr int kRescRow = kLogNB + kLogNB / 2;      // u64 words of a rescued pair's row: 2048 suffix sums (fp64) + 2048 suffix counts (u32)

// Capacity (elements, a multiple of 32: whole 128-byte lines) of the LIST REGION of one slice of n elements in the one-read
// forms' list buffers.  The exact-tail form lists ~0.5 - 1.5 % of a pair (a wave's budget: kTailAllow0 + what it has seen >> 6,
// + 512 per raise) and the rescue gathers a bracket's bins (~2 %): a region holds n / 16 + 16384 values, never more than the
// slice itself.  What does not fit — saturating activations with a tenth of their values at the maximum, constant tensors —
// is not listed: the pair's walk is refused (its list length says so) and it finishes on the compaction route, whose
// full-size lists the caller provides only when a batch reports such pairs.  Round 4 gave every pair a region of its own
// size in every list: 4 x the batch's activations in scratch.  (n / 32 + 16384 was too tight for the rescue: the bracket of a
// cold 802 816-element pair holds 5 - 6 % of it, and 14 pairs of every cold ResNet-50 sweep ended on the compaction route.)
constexpr uint32_t kListCapShift = 4, kListCapConst = 16384;
constexpr uint32_t list_cap_of(unsigned long long n) {
    const unsigned long long whole = (n + 31ull) & ~31ull, part = ((n >> kListCapShift) + kListCapConst + 31ull) & ~31ull;
    return (uint32_t)((whole < part || n <= kSmallCap) ? whole : part);
}

}  // namespace
