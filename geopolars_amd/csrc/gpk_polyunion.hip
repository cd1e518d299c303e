// gpk_polyunion.hip — polygon x polygon union: gpk_polygon_union, the schedule of gpk_polyclip_run.h instantiated with the kept table
// of gpk_polyunion.h and the innermost-shell nesting (its own count, fill and stitch kernels: gpk_polygon_clip launches what it
// launched), and gpk_union_all_pairs, the pairing of one round of a grouped union.  Contract: include/geopolars_hip.h.
#include "gpk_polyclip_run.h"
#include "gpk_polyunion.h"

namespace gpk {

namespace {

// the role of every current row (pu::union_all_role): opens[i] = 1 when row i opens a pair, stays[i] = 1 when row i leaves a row to
// the next round (it opens a pair or passes through).  The first row of a group is found by bisection in the sorted ids.
__global__ __launch_bounds__(256) void union_all_roles_kernel(const int32_t* __restrict__ group, int64_t n, int32_t* __restrict__ opens,
                                                              int32_t* __restrict__ stays) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t g = group[i];
    int64_t lo = 0, hi = i;  // the lowest index whose id is g lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (group[mid] < g) lo = mid + 1; else hi = mid;
    }
    const int role = pu::union_all_role(group, n, i, lo);
    opens[i] = role == 0 ? 1 : 0;
    stays[i] = role != 1 ? 1 : 0;
}

// pair k = pair_at[i] of the row i that opens it: a_rows[k], b_rows[k] = the pool rows of i and i + 1; the row j = next_at[i] of the
// next round: its group, and its pool row — base + k for the result of a pair, the row's own for one that passes through.
__global__ __launch_bounds__(256) void union_all_scatter_kernel(const int32_t* __restrict__ group, const uint32_t* __restrict__ rows, int64_t n,
                                                                int64_t base, const int32_t* __restrict__ opens, const int32_t* __restrict__ stays,
                                                                const int32_t* __restrict__ pair_at, const int32_t* __restrict__ next_at,
                                                                uint32_t* __restrict__ a_rows, uint32_t* __restrict__ b_rows,
                                                                int32_t* __restrict__ next_group, uint32_t* __restrict__ next_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !stays[i]) return;
    const int64_t j = next_at[i];
    if (j >= n) return;  // (cannot happen: at most one row stays per row)
    next_group[j] = group[i];
    if (opens[i] && i + 1 < n) {
        const int64_t k = pair_at[i];
        if (k < n / 2) {  // (always: a pair takes two rows)
            a_rows[k] = rows ? rows[i] : (uint32_t)i;
            b_rows[k] = rows ? rows[i + 1] : (uint32_t)(i + 1);
        }
        next_rows[j] = (uint32_t)(base + k);
    } else {
        next_rows[j] = rows ? rows[i] : (uint32_t)i;
    }
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_polygon_union(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows,
                                     int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status,
                                     int32_t status_space, void* stream, gpk_geoarray** out) {
    static const RunNames names = {"polygon_union",           "gpk_polygon_union_count",   "gpk_polygon_union_fill", "gpk_polygon_union_stitch",
                                   "gpk_polygon_union_totals", "gpk_polygon_union_offsets", "gpk_polygon_union_emit"};
    return polygon_clip_run<pu::UnionRule, true>(names, mode == GPK_PUNION_UNION, a, b, a_rows, b_rows, n_rows, rows_space, mode, flags, out_src,
                                                 src_space, out_status, status_space, stream, out);
}

extern "C" int32_t gpk_union_all_pairs(const int32_t* group, const uint32_t* rows, int64_t n, int64_t base, uint32_t* a_rows, uint32_t* b_rows,
                                       int32_t* next_group, uint32_t* next_rows, int64_t* out_counts, void* stream) {
    if (n < 0 || n > (int64_t)INT32_MAX || base < 0 || base + n / 2 > (int64_t)UINT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "union_all_pairs: %lld rows from pool row %lld", (long long)n, (long long)base);
    if (!out_counts || (n > 0 && (!group || !next_group || !next_rows)) || (n > 1 && (!a_rows || !b_rows)))
        return fail(GPK_ERR_INVALID_ARGUMENT, "union_all_pairs: NULL argument");
    out_counts[0] = out_counts[1] = 0;
    if (n == 0) return GPK_OK;
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const size_t tot = (size_t)((n + 255) / 256 + 2);
    Scratch sc(workspace());
    int32_t *opens, *stays, *pair_at, *next_at;
    unsigned long long *tot_pairs, *tot_next, *totals_dev;
    sc.add_n((size_t)(n + 1), opens, stays, pair_at, next_at);
    sc.add_n(tot, tot_pairs, tot_next);
    sc.add(totals_dev, 64);
    GPK_TRY(sc.commit());
    const dim3 grid((unsigned)((n + 255) / 256));
    const int64_t at = (n + 255) / 256;
    GPK_LAUNCH("gpk_union_all_roles", union_all_roles_kernel, grid, dim3(256), 0, s, group, n, opens, stays);
    GPK_TRY(exclusive_scan_i32(opens, n, pair_at, nullptr, tot_pairs, s));
    GPK_TRY(exclusive_scan_i32(stays, n, next_at, nullptr, tot_next, s));
    GPK_LAUNCH("gpk_union_all_scatter", union_all_scatter_kernel, grid, dim3(256), 0, s, group, rows, n, base, (const int32_t*)opens, (const int32_t*)stays,
               (const int32_t*)pair_at, (const int32_t*)next_at, a_rows, b_rows, next_group, next_rows);
    unsigned long long totals[4] = {0, 0, 0, 0};
    GPK_TRY(clip_read_totals("gpk_union_all_totals", tot_pairs + at, tot_next + at, nullptr, nullptr, totals_dev, totals, s));
    out_counts[0] = (int64_t)totals[0];
    out_counts[1] = (int64_t)totals[1];
    return GPK_OK;
}
