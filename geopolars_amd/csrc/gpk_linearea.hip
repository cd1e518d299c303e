// gpk_linearea.hip — line x polygon relations: the row-wise mask (gpk_line_polygon_relation) and the predicate join
// (gpk_line_polygon_join) over the device routine of gpk_linearea.h.  Contract: include/geopolars_hip.h.
//
// Row-wise: G lanes per row, G = relation_group_size(lines, polys) (4 or 16, from the polygon column's mean coordinate count: the
// lanes stride ring edges).  There is no work-group path for large rows: a pair costs segments x edges box tests, and the 16-lane
// routine is the only schedule.
//
// Join: the staged bbox candidate generator (gpk_candjoin.h) with the left rows' own boxes; the refine runs the same routine with G
// lanes per CANDIDATE and writes hit = predicate(mask).  When the caller asks for the per-pair masks the full mask is computed and
// gathered after the emit; otherwise the walk of a pair ends as soon as its predicate is settled (lp::stop_of).
//
// The host steps around the kernels are shared (gpk_candjoin.h): rowwise_pairs stages a host caller's buffers for the row-wise call,
// payload_join runs the join (temporary index, boxes, bbox_join, the gather of the per-pair values) around this file's refine.
#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_linearea.h"

namespace gpk {

namespace {

template <int G>
__global__ __launch_bounds__(256) void line_polygon_rowwise_kernel(DevGeo lines, DevGeo polys, const uint32_t* __restrict__ rows, int64_t n,
                                                                   uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += groups) {
        const int64_t j = rows ? (int64_t)rows[i] : i;
        const int mask = lp::line_polygon_mask_group<G>(lines, i, polys, j, lane);
        if (lane == 0) out[i] = (uint8_t)mask;
    }
}

struct LpCtx {
    PayloadCtx p;  // (p.payload_out: the masks were asked for)
    int32_t predicate;
};

// G lanes per candidate; `line_left`: the caller's left column holds the lines
template <int G>
__global__ __launch_bounds__(256) void line_polygon_refine_kernel(DevGeo lines, DevGeo polys, bool line_left, const uint32_t* __restrict__ cand_l,
                                                                  const uint32_t* __restrict__ cand_r, int64_t n, int predicate, lp::Stop st,
                                                                  uint8_t* __restrict__ hit, uint8_t* __restrict__ mask_out) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t c = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; c < n; c += groups) {
        const int64_t l = cand_l[c], r = cand_r[c];
        const int mask = lp::line_polygon_mask_group<G>(lines, line_left ? l : r, polys, line_left ? r : l, lane, st);
        if (lane == 0) {
            hit[c] = lp::predicate_of(mask, predicate) ? 1 : 0;
            if (mask_out) mask_out[c] = (uint8_t)mask;
        }
    }
}

// scratch of a call: 256 bytes unused, then mask[n_cand] when the masks were asked for
int32_t lp_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit, unsigned long long* stats,
                  hipStream_t s) {
    (void)stats;
    const LpCtx& cx = *(const LpCtx*)ctx;
    const bool line_left = is_lineal(cx.p.left->d.type);
    const DevGeo &lines = line_left ? cx.p.left->d : cx.p.right->d, &polys = line_left ? cx.p.right->d : cx.p.left->d;
    uint8_t* mask = cx.p.payload_out ? (uint8_t*)scratch + 256 : nullptr;
    const lp::Stop st = mask ? lp::Stop{0, lp::LP_ALL} : lp::stop_of(cx.predicate);
    const int G = lp::relation_group_size(lines, polys);
    const dim3 grid = group_grid(n_cand, G);
    if (G == lp::LP_G_SMALL)
        GPK_LAUNCH("gpk_line_polygon_refine", (line_polygon_refine_kernel<lp::LP_G_SMALL>), grid, dim3(256), 0, s, lines, polys, line_left, cand_l, cand_r,
                   (int64_t)n_cand, (int)cx.predicate, st, hit, mask);
    else
        GPK_LAUNCH("gpk_line_polygon_refine", (line_polygon_refine_kernel<lp::LP_G_LARGE>), grid, dim3(256), 0, s, lines, polys, line_left, cand_l, cand_r,
                   (int64_t)n_cand, (int)cx.predicate, st, hit, mask);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_line_polygon_relation(const gpk_geoarray* lines, const gpk_geoarray* polys, const uint32_t* poly_rows, uint8_t* out_mask,
                                             int32_t out_space, void* stream) {
    if (!lines || !polys || !out_mask) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_lineal(lines->d.type) || !is_polygonal(polys->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "line_polygon_relation: LINESTRING | MULTILINESTRING x POLYGON | MULTIPOLYGON (found types %d, %d)",
                    lines->d.type, polys->d.type);
    auto launch = [&](const uint32_t* rows_dev, void* out_dev, int64_t n, hipStream_t s) -> int32_t {
        const int G = lp::relation_group_size(lines->d, polys->d);
        const dim3 grid = group_grid(n, G);
        if (G == lp::LP_G_SMALL)
            GPK_LAUNCH("gpk_line_polygon_relation", (line_polygon_rowwise_kernel<lp::LP_G_SMALL>), grid, dim3(256), 0, s, lines->d, polys->d, rows_dev, n,
                       (uint8_t*)out_dev);
        else
            GPK_LAUNCH("gpk_line_polygon_relation", (line_polygon_rowwise_kernel<lp::LP_G_LARGE>), grid, dim3(256), 0, s, lines->d, polys->d, rows_dev, n,
                       (uint8_t*)out_dev);
        return GPK_OK;
    };
    return rowwise_pairs("line_polygon_relation", lines, polys, poly_rows, out_mask, 1, out_space, stream, launch);
}

extern "C" int32_t gpk_line_polygon_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t predicate,
                                         uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, uint8_t* out_mask, int64_t pair_capacity,
                                         int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (predicate < GPK_LP_PRED_INTERSECTS || predicate > GPK_LP_PRED_TOUCHES)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_polygon_join: unknown predicate %d", predicate);
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    if (!((is_lineal(left->d.type) && is_polygonal(right->d.type)) || (is_polygonal(left->d.type) && is_lineal(right->d.type))))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "line_polygon_join: one side lineal, the other polygonal (found types %d, %d)", left->d.type,
                    right->d.type);
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "line_polygon_join"));
    LpCtx cx{{left, right, "gpk_line_polygon_gather", sizeof(uint8_t), nullptr}, predicate};
    return payload_join(PayloadJoin{"line_polygon_join", &cx.p, lp_refine, 0, nullptr}, right_index, left_row_base, out_counts, out_pairs, out_mask,
                        pair_capacity, n_pairs, out_space, stream);
}
