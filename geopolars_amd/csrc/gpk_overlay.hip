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
#include <cmath>

#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_overlay.h"

namespace gpk {

namespace {

bool lineal(int32_t t) { return t == GPK_GEOM_LINESTRING || t == GPK_GEOM_MULTILINESTRING; }

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
    const gpk_geoarray *left, *right;
    double min_measure;
    double* measure_out;  // device: out_measure itself or its staging; nullptr: no measures asked for
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

// out_measure: the measures of row i's hits, in candidate order, at the row's offset of the output
__global__ __launch_bounds__(256) void intersection_measure_gather_kernel(int64_t n_rows, const int32_t* __restrict__ cand_off,
                                                                          const uint8_t* __restrict__ hit, const int32_t* __restrict__ offsets,
                                                                          const double* __restrict__ measure, double* __restrict__ out, int64_t capacity) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    int64_t o = offsets[i];
    for (int c = cand_off[i]; c < cand_off[i + 1]; ++c) {
        if (!hit[c]) continue;
        if (o < capacity) out[o] = measure[c];
        ++o;
    }
}

dim3 group_grid(int64_t n, int G) {
    const int64_t per_block = 256 / G;
    int64_t blocks = (n + per_block - 1) / per_block;
    const int64_t cap = (int64_t)cu_count() * 32;
    if (blocks > cap) blocks = cap;
    return dim3((unsigned)(blocks > 0 ? blocks : 1));
}

int group_size(const DevGeo& a, const DevGeo& b) { return lineal(a.type) ? lp::relation_group_size(a, b) : pp::relation_group_size(a, b); }

// scratch of a call: 256 bytes unused, then measure[n_cand] when the measures were asked for
int32_t ov_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit, unsigned long long* stats,
                  hipStream_t s) {
    (void)stats;
    const OvCtx& cx = *(const OvCtx*)ctx;
    const DevGeo &left = cx.left->d, &right = cx.right->d;
    double* measure = cx.measure_out ? (double*)((char*)scratch + 256) : nullptr;
    const int G = group_size(left, right);
    const bool length = lineal(left.type);
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

int32_t ov_emitted(void* ctx, int64_t n_rows, const int32_t* cand_off, const uint8_t* hit, const int32_t* offsets, void* scratch,
                   int64_t pair_capacity, hipStream_t s) {
    const OvCtx& cx = *(const OvCtx*)ctx;
    if (!cx.measure_out) return GPK_OK;
    GPK_LAUNCH("gpk_intersection_measure_gather", intersection_measure_gather_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, n_rows,
               cand_off, hit, offsets, (const double*)((const char*)scratch + 256), cx.measure_out, pair_capacity);
    return GPK_OK;
}

// area for polygonal x polygonal, length for lineal x polygonal; everything else is refused
int32_t check_families(const char* who, int32_t ta, int32_t tb) {
    if ((is_polygonal(ta) || lineal(ta)) && is_polygonal(tb)) return GPK_OK;
    if (is_polygonal(ta) && lineal(tb))
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
    const int64_t n = a->d.n_geoms;
    if (!b_rows && n != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "intersection_measure: row counts differ (%lld vs %lld)", (long long)n, (long long)b->d.n_geoms);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return GPK_OK;
    const uint32_t* rows_dev = b_rows;
    double* out_dev = out;
    const size_t ob = sizeof(double) * (size_t)n;
    if (out_space != GPK_MEM_DEVICE) {
        const size_t rb = sizeof(uint32_t) * (size_t)n;
        GPK_TRY(workspace().begin(align256(ob) + (b_rows ? align256(rb) : 0) + 512));
        out_dev = (double*)workspace().take(ob);
        if (b_rows) {
            uint32_t* r = (uint32_t*)workspace().take(rb);
            GPK_HIP(hipMemcpyAsync(r, b_rows, rb, hipMemcpyHostToDevice, s));
            rows_dev = r;
        }
    }
    const int G = group_size(a->d, b->d);
    const bool length = lineal(a->d.type);
    const dim3 grid = group_grid(n, G);
#define GPK_OV_ROWWISE(GG, LL) \
    GPK_LAUNCH("gpk_intersection_measure", (intersection_measure_rowwise_kernel<GG, LL>), grid, dim3(256), 0, s, a->d, b->d, rows_dev, n, out_dev)
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
    return copy_out(out, out_space, out_dev, ob, s);
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
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = left->d.n_geoms;
    if (n == 0) return GPK_OK;
    if (n > (int64_t)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "intersection_measure_join: more than 2^31 - 1 left rows: shard the left side");
    const bool host_out = out_space != GPK_MEM_DEVICE;
    if (right->d.n_geoms == 0) {  // nothing to meet: every count is zero
        GPK_TRY(zero_counts(out_counts, n, out_space, s));
        if (out_counts && !host_out) GPK_HIP(hipStreamSynchronize(s));
        return GPK_OK;
    }

    gpk_index* tmp_index = nullptr;  // (built before the arenas are carved: the build uses them itself)
    if (!right_index) {
        GPK_TRY(gpk_index_build_ex(right, GPK_INDEX_BBOX_GRID, nullptr, stream, &tmp_index));
        right_index = tmp_index;
    }
    auto finish = [&](int32_t rc) {
        if (tmp_index) {
            (void)hipStreamSynchronize(s);
            gpk_index_free(tmp_index);
        }
        return rc;
    };
    const bool want_measure = out_measure && pair_capacity > 0;
    const size_t box_bytes = sizeof(double4) * (size_t)n, measure_bytes = sizeof(double) * (size_t)pair_capacity;
    int32_t rc = workspace_aux(0).begin(align256(box_bytes) + (want_measure && host_out ? align256(measure_bytes) : 0) + 512);
    if (rc != GPK_OK) return finish(rc);
    double4* lbox = (double4*)workspace_aux(0).take(box_bytes);
    double* measure_dev = want_measure ? (host_out ? (double*)workspace_aux(0).take(measure_bytes) : out_measure) : nullptr;
    rc = gpk_bounds(left, (double*)lbox, GPK_MEM_DEVICE, stream);
    if (rc != GPK_OK) return finish(rc);

    OvCtx cx{left, right, min_measure, measure_dev};
    CandRefine hook;
    hook.name = "intersection_measure_join";
    hook.ctx = &cx;
    hook.scratch_fixed = 512;
    hook.scratch_per_cand = measure_dev ? sizeof(double) : 0;
    hook.refine = ov_refine;
    hook.emitted = ov_emitted;
    rc = bbox_join(left, right, right_index, left_row_base, out_counts, out_pairs, pair_capacity, n_pairs, out_space, s, lbox, hook);
    if (rc != GPK_OK) return finish(rc);
    if (want_measure && host_out && *n_pairs > 0) {
        const int64_t got = *n_pairs < pair_capacity ? *n_pairs : pair_capacity;
        rc = copy_out(out_measure, out_space, measure_dev, sizeof(double) * (size_t)got, s);
    }
    return finish(rc);
}
