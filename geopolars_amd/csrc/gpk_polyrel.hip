// gpk_polyrel.hip — polygon x polygon relations: the row-wise mask (gpk_polygon_relation) and the predicate join
// (gpk_polygon_relation_join) over the device routine of gpk_polyrel.h.  Contract: include/geopolars_hip.h.
//
// Row-wise: G lanes per row, G = pp::relation_group_size(a, b) (4 or 16, from the larger of the two columns' mean coordinate counts:
// the lanes stride the ring edges of either side in turn).  There is no work-group path for large rows: the 16-lane routine is the
// only schedule.
//
// Join: the staged bbox candidate generator (gpk_candjoin.h) with the left rows' own boxes; the refine runs the same routine with G
// lanes per CANDIDATE, A = the left row and B = the right row, and writes hit = predicate(mask).  When the caller asks for the per-pair
// masks the full mask is computed and gathered after the emit; otherwise the work on a pair ends as soon as its predicate is settled
// (pp::stop_of).  `left` and `right` may be one array: a pair (i, i) is a candidate like any other.
//
// The host steps around the kernels are shared (gpk_candjoin.h): rowwise_pairs stages a host caller's buffers for the row-wise call,
// payload_join runs the join (temporary index, boxes, bbox_join, the gather of the per-pair values) around this file's refine.
#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_polyrel.h"

namespace gpk {

namespace {

template <int G>
__global__ __launch_bounds__(256) void polygon_relation_rowwise_kernel(DevGeo a, DevGeo b, const uint32_t* __restrict__ rows, int64_t n,
                                                                       uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += groups) {
        const int64_t j = rows ? (int64_t)rows[i] : i;
        const int mask = pp::polygon_polygon_mask_group<G>(a, i, b, j, lane);
        if (lane == 0) out[i] = (uint8_t)mask;
    }
}

struct PpCtx {
    PayloadCtx p;  // (p.payload_out: the masks were asked for)
    int32_t predicate;
};

// G lanes per candidate
template <int G>
__global__ __launch_bounds__(256) void polygon_relation_refine_kernel(DevGeo left, DevGeo right, const uint32_t* __restrict__ cand_l,
                                                                      const uint32_t* __restrict__ cand_r, int64_t n, int predicate, pp::Stop st,
                                                                      uint8_t* __restrict__ hit, uint8_t* __restrict__ mask_out) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t c = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; c < n; c += groups) {
        const int mask = pp::polygon_polygon_mask_group<G>(left, (int64_t)cand_l[c], right, (int64_t)cand_r[c], lane, st);
        if (lane == 0) {
            hit[c] = pp::predicate_of(mask, predicate) ? 1 : 0;
            if (mask_out) mask_out[c] = (uint8_t)mask;
        }
    }
}

// scratch of a call: 256 bytes unused, then mask[n_cand] when the masks were asked for
int32_t pp_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit, unsigned long long* stats,
                  hipStream_t s) {
    (void)stats;
    const PpCtx& cx = *(const PpCtx*)ctx;
    const DevGeo &left = cx.p.left->d, &right = cx.p.right->d;
    uint8_t* mask = cx.p.payload_out ? (uint8_t*)scratch + 256 : nullptr;
    const pp::Stop st = mask ? pp::Stop{0, pp::PP_ALL} : pp::stop_of(cx.predicate);
    const int G = pp::relation_group_size(left, right);
    const dim3 grid = group_grid(n_cand, G);
    if (G == lp::LP_G_SMALL)
        GPK_LAUNCH("gpk_polygon_relation_refine", (polygon_relation_refine_kernel<lp::LP_G_SMALL>), grid, dim3(256), 0, s, left, right, cand_l, cand_r,
                   (int64_t)n_cand, (int)cx.predicate, st, hit, mask);
    else
        GPK_LAUNCH("gpk_polygon_relation_refine", (polygon_relation_refine_kernel<lp::LP_G_LARGE>), grid, dim3(256), 0, s, left, right, cand_l, cand_r,
                   (int64_t)n_cand, (int)cx.predicate, st, hit, mask);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_polygon_relation(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, uint8_t* out_mask, int32_t out_space,
                                        void* stream) {
    if (!a || !b || !out_mask) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_polygonal(a->d.type) || !is_polygonal(b->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "polygon_relation: POLYGON | MULTIPOLYGON x POLYGON | MULTIPOLYGON (found types %d, %d)", a->d.type,
                    b->d.type);
    auto launch = [&](const uint32_t* rows_dev, void* out_dev, int64_t n, hipStream_t s) -> int32_t {
        const int G = pp::relation_group_size(a->d, b->d);
        const dim3 grid = group_grid(n, G);
        if (G == lp::LP_G_SMALL)
            GPK_LAUNCH("gpk_polygon_relation", (polygon_relation_rowwise_kernel<lp::LP_G_SMALL>), grid, dim3(256), 0, s, a->d, b->d, rows_dev, n,
                       (uint8_t*)out_dev);
        else
            GPK_LAUNCH("gpk_polygon_relation", (polygon_relation_rowwise_kernel<lp::LP_G_LARGE>), grid, dim3(256), 0, s, a->d, b->d, rows_dev, n,
                       (uint8_t*)out_dev);
        return GPK_OK;
    };
    return rowwise_pairs("polygon_relation", a, b, b_rows, out_mask, 1, out_space, stream, launch);
}

extern "C" int32_t gpk_polygon_relation_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t predicate,
                                             uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, uint8_t* out_mask,
                                             int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (predicate < GPK_PP_PRED_INTERSECTS || predicate > GPK_PP_PRED_CONTAINS_PROPERLY)
        return fail(GPK_ERR_INVALID_ARGUMENT, "polygon_relation_join: unknown predicate %d", predicate);
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    if (!is_polygonal(left->d.type) || !is_polygonal(right->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "polygon_relation_join: both sides POLYGON | MULTIPOLYGON (found types %d, %d)", left->d.type,
                    right->d.type);
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "polygon_relation_join"));
    PpCtx cx{{left, right, "gpk_polygon_relation_gather", sizeof(uint8_t), nullptr}, predicate};
    return payload_join(PayloadJoin{"polygon_relation_join", &cx.p, pp_refine, 0, nullptr}, right_index, left_row_base, out_counts, out_pairs, out_mask,
                        pair_capacity, n_pairs, out_space, stream);
}
