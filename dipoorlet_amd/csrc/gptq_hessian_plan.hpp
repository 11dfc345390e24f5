// HOST side of the device Hessian (gptq_hessian_kernels.hip), defined once — pure arithmetic, no HIP: how the rows of X are cut
// into ranges (gh_plan), the size of the partial-tile workspace, and the argument rules of dpl_gptq_hessian in their order
// (gh_check).  A wrong value here is an out-of-range address in a kernel, so a plain C++ compiler can build this.
#pragma once
#include <stdint.h>

#include "../../include/dipoorlet_hip.h"
#include "gptq_factor_plan.hpp"
#include "host_error.hpp"

namespace {

constexpr int kGhPass = 32;                    // rows of X staged per pass: every range begins on a multiple of it
// The row split.  A workgroup holds 40 KiB of LDS, so a compute unit of 160 KiB keeps four, and 256 compute units 1024: the split
// aims at that many workgroups — one resident round, no second round that a few stragglers would stretch.
constexpr uint32_t kGhTargetGroups = 1024;
// ... with a floor on the rows of a range: a workgroup reads 2 panels x 64 columns x 4 bytes = 512 bytes of X per row, and its
// partial tile costs 32 KiB written and 32 KiB read back.  At 1024 rows the partial traffic is 64 KiB against 512 KiB: an eighth.
constexpr uint32_t kGhMinRows = 1024;
constexpr int64_t kGhMaxRows = 0x7FFFFFFF - kGhPass;       // row indices and their round-up stay inside 32 bits
constexpr uint64_t kGhTileBytes = (uint64_t)kGfB * kGfB * sizeof(double);

// Range s < splits is rows [s * range_rows, min(rows, (s + 1) * range_rows)): range_rows is a multiple of 32 and no range is empty.
// splits depends on (rows, k) alone.  splits == 1: no workspace, the tile kernel adds onto H itself.
struct GhPlan {
    uint32_t k, rows, nt, tiles;      // nt = ceil(k / 64); tiles on and below the diagonal
    uint32_t splits, range_rows;
    uint64_t bytes;                   // of the workspace: splits * tiles partial tiles of 64 x 64 doubles, or 0
    uint32_t begin(uint32_t s) const { return s * range_rows; }
    uint32_t end(uint32_t s) const { return s + 1 == splits ? rows : (s + 1) * range_rows; }
};

inline GhPlan gh_plan(int64_t k, int64_t rows) {      // 1 <= k <= DPL_GPTQ_FACTOR_MAX_K, 1 <= rows <= kGhMaxRows
    GhPlan p;
    p.k = (uint32_t)k;
    p.rows = (uint32_t)rows;
    p.nt = (p.k + kGfB - 1) / kGfB;
    p.tiles = GfPlan::lower(p.nt);
    uint32_t want = (kGhTargetGroups + p.tiles - 1) / p.tiles;
    const uint32_t most = p.rows / kGhMinRows;
    if (want > most) want = most;
    if (want < 1) want = 1;
    const uint32_t per = (p.rows + want - 1) / want;
    p.range_rows = (per + kGhPass - 1) / kGhPass * kGhPass;
    p.splits = (p.rows + p.range_rows - 1) / p.range_rows;       // (<= want: rounding the ranges up can only empty the last ones)
    p.bytes = p.splits > 1 ? (uint64_t)p.splits * p.tiles * kGhTileBytes : 0;
    return p;
}

// The conv form's view of x [batch, channels, height, width]: the output extent per axis, or <= 0 when the window does not fit.
inline int64_t gh_out(int64_t padded, int64_t kernel, int64_t stride, int64_t dil) {
    const int64_t last = padded - dil * (kernel - 1) - 1;      // where the last window may begin
    return last < 0 ? 0 : last / stride + 1;
}
inline int64_t gh_out_h(const dpl_gptq_hessian_geom& g) { return gh_out(g.height + g.pad_top + g.pad_bottom, g.kh, g.stride_h, g.dil_h); }
inline int64_t gh_out_w(const dpl_gptq_hessian_geom& g) { return gh_out(g.width + g.pad_left + g.pad_right, g.kw, g.stride_w, g.dil_w); }

// -> 0, or the refusal (-2, nothing launched).  geom == nullptr: the dense form.
inline int gh_check(const void* d_x, const dpl_gptq_hessian_geom* geom, int64_t k, int64_t rows, const void* d_h, const void* d_workspace,
                    uint64_t workspace_bytes) {
    if (d_x == nullptr || d_h == nullptr) return fail_msg("dpl_gptq_hessian: null pointer");
    if (k < 1 || k > DPL_GPTQ_FACTOR_MAX_K) return fail_msg("dpl_gptq_hessian: k must be in [1, 16384]");
    if (rows < 0 || rows > kGhMaxRows) return fail_msg("dpl_gptq_hessian: rows must be in [0, 2^31 - 33]");
    if (geom != nullptr) {
        const dpl_gptq_hessian_geom& g = *geom;
        if (g.batch < 1 || g.channels < 1 || g.height < 1 || g.width < 1 || g.kh < 1 || g.kw < 1 || g.stride_h < 1 || g.stride_w < 1 ||
            g.dil_h < 1 || g.dil_w < 1 || g.pad_top < 0 || g.pad_left < 0 || g.pad_bottom < 0 || g.pad_right < 0)
            return fail_msg("dpl_gptq_hessian: the geometry needs positive sizes, strides and dilations and pads >= 0");
        if (g.channels > k || g.kh > k || g.kw > k || g.channels * g.kh * g.kw != k)
            return fail_msg("dpl_gptq_hessian: k is not channels * kh * kw of the geometry");
        // (what the kernel keeps in 15 bits: a padded axis and a window's reach along it; in 32: an image's elements)
        const int64_t lim = 0x7FFF;
        if (g.height > lim || g.width > lim || g.pad_top > lim || g.pad_left > lim || g.pad_bottom > lim || g.pad_right > lim ||
            g.dil_h > lim || g.dil_w > lim || g.stride_h > lim || g.stride_w > lim || g.height + g.pad_top + g.pad_bottom > lim ||
            g.width + g.pad_left + g.pad_right > lim || g.dil_h * (g.kh - 1) > lim || g.dil_w * (g.kw - 1) > lim ||
            g.channels * g.height * g.width + g.dil_h * (g.kh - 1) * g.width + g.dil_w * (g.kw - 1) > 0x7FFFFFFF)
            return fail_msg("dpl_gptq_hessian: the geometry is beyond the kernel's index widths (an image of 2^31 elements, an axis of 2^15)");
        if (gh_out_h(g) < 1 || gh_out_w(g) < 1) return fail_msg("dpl_gptq_hessian: the output extent of the geometry is not positive");
        if (g.batch > rows || g.batch * gh_out_h(g) * gh_out_w(g) != rows)
            return fail_msg("dpl_gptq_hessian: rows is not batch * out_h * out_w of the geometry");
    }
    if (rows == 0) return 0;
    const GhPlan p = gh_plan(k, rows);
    if (p.bytes > 0 && d_workspace == nullptr) return fail_msg("dpl_gptq_hessian: null pointer (the workspace)");
    if (workspace_bytes < p.bytes) return fail_msg("dpl_gptq_hessian: the workspace is smaller than dpl_gptq_hessian_workspace(k, rows)");
    return 0;
}

}  // namespace
