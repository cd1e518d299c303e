// gpk_overlay.hip — how much two geometries share: the row-wise measure (gpk_intersection_measure) and the measure join
// (gpk_intersection_measure_join) over the device routines of gpk_overlay.h.  Contract: include/geopolars_hip.h.
//
// Row-wise: G lanes per row, G = pp::relation_group_size(a, b) for two polygonal columns (the area), lp::relation_group_size(lines,
// polys) for lines against polygons (the length).  There is no work-group path for large rows: the 16-lane routine is the only
// schedule, the limit gpk_polyrel.hip states.
//
// Join: the staged bbox candidate generator (gpk_candjoin.h) with the left rows' own boxes; the refine runs the same routine with G
// lanes per CANDIDATE and writes hit = measure > min_measure (on doubles; NaN never hits).  The per-pair measures are kept per
// candidate and gathered after the emit.  Same routine, same G, same lane order: a pair's measure is bit for bit the row-wise one.
//
// The host steps around the kernels are shared (gpk_candjoin.h): rowwise_pairs stages a host caller's buffers for the row-wise call,
// payload_join runs the join (temporary index, boxes, bbox_join, the gather of the per-pair values) around this file's refine.
#include <cmath>

#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_overlay.h"

namespace gpk {

namespace {

template <int G, bool LENGTH>
__device__ __forceinline__ double measure_group(const DevGeo& a, int64_t i, const DevGeo& b, int64_t j, int lane) {
    if constexpr (LENGTH)
        return ov::intersection_length_group<G>(a, i, b, j, lane);
    else
        return ov::intersection_area_group<G>(a, i, b, j, lane);
}

template <int G, bool LENGTH>
__global__ __launch_bounds__(256) void intersection_measure_rowwise_kernel(DevGeo a, DevGeo b, const uint32_t* __restrict__ rows, int64_t n,
                                                                           double* __restrict__ out) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += groups) {
        const int64_t j = rows ? (int64_t)rows[i] : i;
        const double m = measure_group<G, LENGTH>(a, i, b, j, lane);
        if (lane == 0) out[i] = m;
    }
}

struct OvCtx {
    PayloadCtx p;  // (p.payload_out: the measures were asked for)
    double min_measure;
};

// G lanes per candidate
template <int G, bool LENGTH>
__global__ __launch_bounds__(256) void intersection_measure_refine_kernel(DevGeo left, DevGeo right, const uint32_t* __restrict__ cand_l,
                                                                          const uint32_t* __restrict__ cand_r, int64_t n, double min_measure,
                                                                          uint8_t* __restrict__ hit, double* __restrict__ measure) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t c = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; c < n; c += groups) {
        const double m = measure_group<G, LENGTH>(left, (int64_t)cand_l[c], right, (int64_t)cand_r[c], lane);
        if (lane == 0) {
            hit[c] = m > min_measure ? 1 : 0;
            if (measure) measure[c] = m;
        }
    }
}

int group_size(const DevGeo& a, const DevGeo& b) { return is_lineal(a.type) ? lp::relation_group_size(a, b) : pp::relation_group_size(a, b); }

// scratch of a call: 256 bytes unused, then measure[n_cand] when the measures were asked for
int32_t ov_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit, unsigned long long* stats,
                  hipStream_t s) {
    (void)stats;
    const OvCtx& cx = *(const OvCtx*)ctx;
    const DevGeo &left = cx.p.left->d, &right = cx.p.right->d;
    double* measure = cx.p.payload_out ? (double*)((char*)scratch + 256) : nullptr;
    const int G = group_size(left, right);
    const bool length = is_lineal(left.type);
    const dim3 grid = group_grid(n_cand, G);
#define GPK_OV_REFINE(GG, LL)                                                                                                                  \
    GPK_LAUNCH("gpk_intersection_measure_refine", (intersection_measure_refine_kernel<GG, LL>), grid, dim3(256), 0, s, left, right, cand_l, cand_r, \
               (int64_t)n_cand, cx.min_measure, hit, measure)
    if (G == lp::LP_G_SMALL) {
        if (length)
            GPK_OV_REFINE(lp::LP_G_SMALL, true);
        else
            GPK_OV_REFINE(lp::LP_G_SMALL, false);
    } else {
        if (length)
            GPK_OV_REFINE(lp::LP_G_LARGE, true);
        else
            GPK_OV_REFINE(lp::LP_G_LARGE, false);
    }
#undef GPK_OV_REFINE
    return GPK_OK;
}

// area for polygonal x polygonal, length for lineal x polygonal; everything else is refused
int32_t check_families(const char* who, int32_t ta, int32_t tb) {
    if ((is_polygonal(ta) || is_lineal(ta)) && is_polygonal(tb)) return GPK_OK;
    if (is_polygonal(ta) && is_lineal(tb))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "%s: the lineal column comes first: swap the arguments (found types %d, %d)", who, ta, tb);
    return fail(GPK_ERR_MISMATCHED_GEOMETRY,
                "%s: POLYGON | MULTIPOLYGON x POLYGON | MULTIPOLYGON (area) or LINESTRING | MULTILINESTRING x POLYGON | MULTIPOLYGON (length) "
                "(found types %d, %d)",
                who, ta, tb);
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_intersection_measure(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double* out, int32_t out_space,
                                            void* stream) {
    if (!a || !b || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    GPK_TRY(check_families("intersection_measure", a->d.type, b->d.type));
    auto launch = [&](const uint32_t* rows_dev, void* out_dev, int64_t n, hipStream_t s) -> int32_t {
        const int G = group_size(a->d, b->d);
        const bool length = is_lineal(a->d.type);
        const dim3 grid = group_grid(n, G);
#define GPK_OV_ROWWISE(GG, LL)                                                                                                               \
    GPK_LAUNCH("gpk_intersection_measure", (intersection_measure_rowwise_kernel<GG, LL>), grid, dim3(256), 0, s, a->d, b->d, rows_dev, n, \
               (double*)out_dev)
        if (G == lp::LP_G_SMALL) {
            if (length)
                GPK_OV_ROWWISE(lp::LP_G_SMALL, true);
            else
                GPK_OV_ROWWISE(lp::LP_G_SMALL, false);
        } else {
            if (length)
                GPK_OV_ROWWISE(lp::LP_G_LARGE, true);
            else
                GPK_OV_ROWWISE(lp::LP_G_LARGE, false);
        }
#undef GPK_OV_ROWWISE
        return GPK_OK;
    };
    return rowwise_pairs("intersection_measure", a, b, b_rows, out, sizeof(double), out_space, stream, launch);
}

extern "C" int32_t gpk_intersection_measure_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index,
                                                 double min_measure, uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs,
                                                 double* out_measure, int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!(min_measure >= 0.0) || std::isinf(min_measure))  // (looked at first: a bad threshold is refused whatever else is handed over)
        return fail(GPK_ERR_INVALID_ARGUMENT, "intersection_measure_join: min_measure must be finite and >= 0, got %g", min_measure);
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    GPK_TRY(check_families("intersection_measure_join", left->d.type, right->d.type));
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "intersection_measure_join"));
    OvCtx cx{{left, right, "gpk_intersection_measure_gather", sizeof(double), nullptr}, min_measure};
    return payload_join(PayloadJoin{"intersection_measure_join", &cx.p, ov_refine, 0, nullptr}, right_index, left_row_base, out_counts, out_pairs,
                        out_measure, pair_capacity, n_pairs, out_space, stream);
}
