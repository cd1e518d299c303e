// gpk_lineline.hip — line x line relations: the row-wise mask (gpk_line_relation) and the predicate join
// (gpk_line_relation_join) over the device routine of gpk_lineline.h.  Contract: include/geopolars_hip.h.
//
// Row-wise: G lanes per row, G = ll::relation_group_size(a, b) (4 or 16, from the larger of the two columns' mean coordinate counts:
// the lanes stride the coordinates of either side in turn).  There is no work-group path for large rows: the 16-lane routine is the
// only schedule.
//
// Join: the staged bbox candidate generator (gpk_candjoin.h) with the left rows' own boxes; the refine runs the same routine with G
// lanes per CANDIDATE, A = the left row and B = the right row, and writes hit = predicate(mask).  When the caller asks for the per-pair
// masks the full mask is computed and gathered after the emit; otherwise the work on a pair ends as soon as its predicate is settled
// (ll::stop_of).  `left` and `right` may be one array: a pair (i, i) is a candidate like any other.
#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_lineline.h"

namespace gpk {

namespace {

bool lineal(int32_t t) { return t == GPK_GEOM_LINESTRING || t == GPK_GEOM_MULTILINESTRING; }

template <int G>
__global__ __launch_bounds__(256) void line_relation_rowwise_kernel(DevGeo a, DevGeo b, const uint32_t* __restrict__ rows, int64_t n,
                                                                       uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += groups) {
        const int64_t j = rows ? (int64_t)rows[i] : i;
        const int mask = ll::line_line_mask_group<G>(a, i, b, j, lane);
        if (lane == 0) out[i] = (uint8_t)mask;
    }
}

struct LlCtx {
    const gpk_geoarray *left, *right;
    int32_t predicate;
    uint8_t* mask_out;  // device: out_mask itself or its staging; nullptr: no masks asked for
};

// G lanes per candidate
template <int G>
__global__ __launch_bounds__(256) void line_relation_refine_kernel(DevGeo left, DevGeo right, const uint32_t* __restrict__ cand_l,
                                                                      const uint32_t* __restrict__ cand_r, int64_t n, int predicate, ll::Stop st,
                                                                      uint8_t* __restrict__ hit, uint8_t* __restrict__ mask_out) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t c = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; c < n; c += groups) {
        const int mask = ll::line_line_mask_group<G>(left, (int64_t)cand_l[c], right, (int64_t)cand_r[c], lane, st);
        if (lane == 0) {
            hit[c] = ll::predicate_of(mask, predicate) ? 1 : 0;
            if (mask_out) mask_out[c] = (uint8_t)mask;
        }
    }
}

// out_mask: the masks of row i's hits, in candidate order, at the row's offset of the output
__global__ __launch_bounds__(256) void line_relation_gather_kernel(int64_t n_rows, const int32_t* __restrict__ cand_off,
                                                                      const uint8_t* __restrict__ hit, const int32_t* __restrict__ offsets,
                                                                      const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, int64_t capacity) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    int64_t o = offsets[i];
    for (int c = cand_off[i]; c < cand_off[i + 1]; ++c) {
        if (!hit[c]) continue;
        if (o < capacity) out[o] = mask[c];
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

// scratch of a call: 256 bytes unused, then mask[n_cand] when the masks were asked for
int32_t ll_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit, unsigned long long* stats,
                  hipStream_t s) {
    (void)stats;
    const LlCtx& cx = *(const LlCtx*)ctx;
    const DevGeo &left = cx.left->d, &right = cx.right->d;
    uint8_t* mask = cx.mask_out ? (uint8_t*)scratch + 256 : nullptr;
    const ll::Stop st = mask ? ll::Stop{0, ll::LL_ALL} : ll::stop_of(cx.predicate);
    const int G = ll::relation_group_size(left, right);
    const dim3 grid = group_grid(n_cand, G);
    if (G == lp::LP_G_SMALL)
        GPK_LAUNCH("gpk_line_relation_refine", (line_relation_refine_kernel<lp::LP_G_SMALL>), grid, dim3(256), 0, s, left, right, cand_l, cand_r,
                   (int64_t)n_cand, (int)cx.predicate, st, hit, mask);
    else
        GPK_LAUNCH("gpk_line_relation_refine", (line_relation_refine_kernel<lp::LP_G_LARGE>), grid, dim3(256), 0, s, left, right, cand_l, cand_r,
                   (int64_t)n_cand, (int)cx.predicate, st, hit, mask);
    return GPK_OK;
}

int32_t ll_emitted(void* ctx, int64_t n_rows, const int32_t* cand_off, const uint8_t* hit, const int32_t* offsets, void* scratch,
                   int64_t pair_capacity, hipStream_t s) {
    const LlCtx& cx = *(const LlCtx*)ctx;
    if (!cx.mask_out) return GPK_OK;
    GPK_LAUNCH("gpk_line_relation_gather", line_relation_gather_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, n_rows, cand_off,
               hit, offsets, (const uint8_t*)scratch + 256, cx.mask_out, pair_capacity);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_line_relation(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, uint8_t* out_mask, int32_t out_space,
                                        void* stream) {
    if (!a || !b || !out_mask) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!lineal(a->d.type) || !lineal(b->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "line_relation: LINESTRING | MULTILINESTRING x LINESTRING | MULTILINESTRING (found types %d, %d)", a->d.type,
                    b->d.type);
    const int64_t n = a->d.n_geoms;
    if (!b_rows && n != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_relation: row counts differ (%lld vs %lld)", (long long)n, (long long)b->d.n_geoms);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return GPK_OK;
    const uint32_t* rows_dev = b_rows;
    uint8_t* out_dev = out_mask;
    if (out_space != GPK_MEM_DEVICE) {
        const size_t rb = sizeof(uint32_t) * (size_t)n;
        GPK_TRY(workspace().begin(align256((size_t)n) + (b_rows ? align256(rb) : 0) + 512));
        out_dev = (uint8_t*)workspace().take((size_t)n);
        if (b_rows) {
            uint32_t* r = (uint32_t*)workspace().take(rb);
            GPK_HIP(hipMemcpyAsync(r, b_rows, rb, hipMemcpyHostToDevice, s));
            rows_dev = r;
        }
    }
    const int G = ll::relation_group_size(a->d, b->d);
    const dim3 grid = group_grid(n, G);
    if (G == lp::LP_G_SMALL)
        GPK_LAUNCH("gpk_line_relation", (line_relation_rowwise_kernel<lp::LP_G_SMALL>), grid, dim3(256), 0, s, a->d, b->d, rows_dev, n, out_dev);
    else
        GPK_LAUNCH("gpk_line_relation", (line_relation_rowwise_kernel<lp::LP_G_LARGE>), grid, dim3(256), 0, s, a->d, b->d, rows_dev, n, out_dev);
    return copy_out(out_mask, out_space, out_dev, (size_t)n, s);
}

extern "C" int32_t gpk_line_relation_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t predicate,
                                             uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, uint8_t* out_mask,
                                             int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (predicate < GPK_LL_PRED_INTERSECTS || predicate > GPK_LL_PRED_EQUALS)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_relation_join: unknown predicate %d", predicate);
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    if (!lineal(left->d.type) || !lineal(right->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "line_relation_join: both sides LINESTRING | MULTILINESTRING (found types %d, %d)", left->d.type,
                    right->d.type);
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "line_relation_join"));
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = left->d.n_geoms;
    if (n == 0) return GPK_OK;
    if (n > (int64_t)INT32_MAX) return fail(GPK_ERR_INVALID_ARGUMENT, "line_relation_join: more than 2^31 - 1 left rows: shard the left side");
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
    const bool want_mask = out_mask && pair_capacity > 0;
    const size_t box_bytes = sizeof(double4) * (size_t)n, mask_bytes = (size_t)pair_capacity;
    int32_t rc = workspace_aux(0).begin(align256(box_bytes) + (want_mask && host_out ? align256(mask_bytes) : 0) + 512);
    if (rc != GPK_OK) return finish(rc);
    double4* lbox = (double4*)workspace_aux(0).take(box_bytes);
    uint8_t* mask_dev = want_mask ? (host_out ? (uint8_t*)workspace_aux(0).take(mask_bytes) : out_mask) : nullptr;
    rc = gpk_bounds(left, (double*)lbox, GPK_MEM_DEVICE, stream);
    if (rc != GPK_OK) return finish(rc);

    LlCtx cx{left, right, predicate, mask_dev};
    CandRefine hook;
    hook.name = "line_relation_join";
    hook.ctx = &cx;
    hook.scratch_fixed = 512;
    hook.scratch_per_cand = mask_dev ? 1 : 0;
    hook.refine = ll_refine;
    hook.emitted = ll_emitted;
    rc = bbox_join(left, right, right_index, left_row_base, out_counts, out_pairs, pair_capacity, n_pairs, out_space, s, lbox, hook);
    if (rc != GPK_OK) return finish(rc);
    if (want_mask && host_out && *n_pairs > 0) rc = copy_out(out_mask, out_space, mask_dev, (size_t)*n_pairs, s);
    return finish(rc);
}
