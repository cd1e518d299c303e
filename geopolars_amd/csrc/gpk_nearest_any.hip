// gpk_nearest_any.hip — nearest-neighbour join (GeoPandas sjoin_nearest) for any two of POINT, MULTIPOINT, LINESTRING, MULTILINESTRING,
// POLYGON and MULTIPOLYGON: for every left row the right rows at the row's minimum distance, ties included.  Contract:
// include/geopolars_hip.h (gpk_nearest_join_any).  gpk_nearest_join (gpk_nearest.hip, POINT left only) is untouched; for a POINT left
// column the two return the same bytes.
//
// Pipeline (payload_join of gpk_candjoin.h: its `boxes` hook does steps 1-3, its refine steps 4-5):
//   1. seed walk (nearest_any_seed_kernel, the rule of gpk_nearwalk.h, one lane per left row): the right row whose BOX is nearest to the
//      left row's box, from the directory alone — no coordinate is read.  No usable box within max_distance + margin: no seed.
//   2. seed distance U_l = d(l, seed_l): the refine kernels of step 4 over the n "candidates" (l, seed_l).
//   3. the left box grown on every side by r_l + margin, r_l = min(U_l, max_distance) (nearest_any_grow_kernel); no seed: a NaN box,
//      which lists no candidates.
//   4. candidates (the staged bbox candidate generator) and their exact distances: the per-candidate kernels of gpk_dwithin.hip with
//      r_l as the threshold of the box pre-test (gpk_dwithin_refine.h) — point_geom_distance<G, KIND> when a side is POINT,
//      pair_distance_group<G, KA, KB> otherwise, the work-group routine above PD_LARGE_COST in a second launch.  These are the routines,
//      group sizes and lane orders of gpk_distance_rowwise's per-row kernels: d is bit for bit the double that call returns.
//   5. per left row the minimum of its candidates' d <= r_l (an atomic minimum on the bits of the non-negative double: a minimum does
//      not depend on the order it is taken in), then hit = (d == minimum); the generator's count / scan / emit and the payload gather
//      give counts, pairs sorted by (l, r) and distances.
//
// Why no nearest row is lost.  Let r* be a right row at the computed minimum d* of row l.  The seed is a usable row, so d* <= U_l, and
// d* <= max_distance or the row has no pair: d* <= r_l.  From here the margin argument at the top of gpk_dwithin.hip carries over with
// r_l in `distance`'s place: the boxes are exact, the gap between them along either axis is at most the exact distance D, and
// |d - D| <= 16 u (D + 2 lmax), so the right box's edge lies within the left box grown by
//   g = fl(r_l + m),   m = 64 eps (|x0| + |y0| + extent width + extent height + |minx| + |miny| + |maxx| + |maxy| + r_l),
// which covers the error of d, the rounding of the grown edge and of g several times over.  The candidate generator compares the grown
// box with the right boxes and assigns cells with the directory's own monotone cell function, exactly.  The refine's box pre-test uses
// the same form of margin around r_l.  A candidate it rejects has a box farther than r_l + margin and so a distance above r_l.
//
// The seed only sets the radius.  Any usable right row would do: the result is the set of rows at the minimum over ALL candidates
// within r_l, and every row at the minimum is a candidate whatever U_l >= d* was.  A worse seed lists more candidates and costs more
// exact evaluations, nothing else.  The known bad case: a left row that lies inside the box of a long diagonal right row gets that row
// as its seed (box distance 0) although the row itself runs far away; r_l is then that far distance and every right row within it is
// evaluated.  The result does not depend on scheduling either: the walk is sequential per row, the distances are those of fixed lane
// orders, and the minimum is order-free.
//
// Never matched: null rows, rows without a coordinate and POINT rows with a NaN coordinate have a NaN box (or are refused by the
// candidate kernels' validity test): no seed on the left, never a seed or a candidate on the right.
#include <cfloat>
#include <cmath>

#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_dwithin_refine.h"
#include "gpk_nearwalk.h"

namespace gpk {

namespace {

constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

// the right side's directory as gpk_nearwalk.h reads it
struct SeedDir {
    const double4* bbox;
    const int32_t* cell_off;
    const int32_t* items;
    const uint8_t* validity;
    __device__ __forceinline__ int cell_begin(int c) const { return cell_off[c]; }
    __device__ __forceinline__ int cell_end(int c) const { return cell_off[c + 1]; }
    __device__ __forceinline__ uint32_t item(int k) const { return (uint32_t)items[k]; }
    __device__ __forceinline__ bool usable(uint32_t j) const { return dev::valid_row(validity, j); }
    __device__ __forceinline__ nw::Box box(uint32_t j) const {
        const double4 b = bbox[j];
        return nw::Box{b.x, b.y, b.z, b.w};
    }
};

// Step 1.  One lane per left row (the walk is sequential and reads only boxes and directory lists).  Writes the row's "candidate"
// (i, seed) and the threshold of its seed distance: INFINITY (always evaluated), or NaN with right row 0 when there is no seed (never
// evaluated; the right side has a row 0: an empty right side returns before this).
__global__ __launch_bounds__(256) void nearest_any_seed_kernel(nw::Grid g, SeedDir dir, const double4* __restrict__ lbox,
                                                               const uint8_t* __restrict__ lvalid, int64_t n, double max_d,
                                                               uint32_t* __restrict__ cand_l, uint32_t* __restrict__ cand_r, double* __restrict__ t_seed) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t seed = nw::NO_SEED;
    if (dev::valid_row(lvalid, i)) {
        const double4 b = lbox[i];
        double bd;
        seed = nw::seed_walk(g, dir, nw::Box{b.x, b.y, b.z, b.w}, max_d, &bd);
    }
    cand_l[i] = (uint32_t)i;
    cand_r[i] = seed == nw::NO_SEED ? 0u : seed;
    t_seed[i] = seed == nw::NO_SEED ? NAN : INFINITY;
}

// Step 3.  (dwithin_grow_kernel with the radius of the row in `distance`'s place; a row without a seed has u = NaN.)
__global__ __launch_bounds__(256) void nearest_any_grow_kernel(const double4* __restrict__ in, const double* __restrict__ u, int64_t n, double max_d,
                                                               double scale, double* __restrict__ radius, unsigned long long* __restrict__ min_bits,
                                                               double4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double ui = u[i];
    const double r = ui == ui ? fmin(ui, max_d) : NAN;  // (fmin would drop the NaN)
    radius[i] = r;
    min_bits[i] = INF_BITS;
    const double4 b = in[i];
    const double m = 64.0 * DBL_EPSILON * (scale + fabs(b.x) + fabs(b.y) + fabs(b.z) + fabs(b.w) + r);
    const double g = r + m;
    out[i] = make_double4(b.x - g, b.y - g, b.z + g, b.w + g);  // (NaN radius or NaN box: a NaN box, no candidates)
}

// Step 5.  Distances are >= 0 (d + 0.0 turns a -0.0 into +0.0), so their order is the order of their bits.
__global__ __launch_bounds__(256) void nearest_any_min_kernel(const uint32_t* __restrict__ cand_l, const double* __restrict__ dist,
                                                              const double* __restrict__ radius, int64_t n_cand, unsigned long long* __restrict__ min_bits) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const uint32_t l = cand_l[c];
    const double d = dist[c];
    if (d <= radius[l]) atomicMin(min_bits + l, (unsigned long long)__double_as_longlong(d + 0.0));  // (false for a NaN on either side)
}
__global__ __launch_bounds__(256) void nearest_any_hit_kernel(const uint32_t* __restrict__ cand_l, const double* __restrict__ dist,
                                                              const double* __restrict__ radius, const unsigned long long* __restrict__ min_bits,
                                                              int64_t n_cand, uint8_t* __restrict__ hit) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const uint32_t l = cand_l[c];
    const double d = dist[c];
    hit[c] = d <= radius[l] && d == __longlong_as_double((long long)min_bits[l]) ? 1 : 0;  // (r_l <= max_distance)
}

struct NaCtx {
    PayloadCtx p;  // (p.payload_out: the distances were asked for)
    double max_d;
    bool pair_kernels;
    const double4 *lbox, *rbox;  // set by nearest_any_boxes
    // per left row, one block allocated by the entry point
    double *radius, *u_seed, *t_seed;
    unsigned long long* min_bits;
    uint32_t *seed_l, *seed_r, *seed_large, *seed_n_large;
    uint8_t* seed_hit;
};

inline dim3 per_element(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// steps 1-3
int32_t nearest_any_boxes(PayloadCtx* ctx, const gpk_index* right_index, const double4* own, double4* grown, int64_t n, hipStream_t s) {
    NaCtx& cx = *(NaCtx*)ctx;
    cx.lbox = own;
    cx.rbox = right_index->v.bbox;
    const GridParams& h = right_index->host_grid;
    const nw::Grid g = nw::make_grid(h.x0, h.y0, h.inv_w, h.inv_h, h.gx, h.gy);
    const SeedDir dir{right_index->v.bbox, right_index->v.cell_off, right_index->v.items, cx.p.right->d.validity};
    GPK_LAUNCH("gpk_nearest_any_seed", nearest_any_seed_kernel, per_element(n), dim3(256), 0, s, g, dir, own, cx.p.left->d.validity, n, cx.max_d,
               cx.seed_l, cx.seed_r, cx.t_seed);
    const RowCands seeds{cx.seed_l, cx.seed_r, n, own, cx.rbox, cx.t_seed, cx.seed_hit, cx.u_seed, nullptr, "gpk_nearest_any_seed_refine",
                         "gpk_nearest_any_seed_refine_large"};
    GPK_TRY(refine_row_candidates("nearest_join_any", cx.p.left, cx.p.right, seeds, cx.seed_large, cx.seed_n_large, s));
    GPK_LAUNCH("gpk_nearest_any_grow", nearest_any_grow_kernel, per_element(n), dim3(256), 0, s, own, (const double*)cx.u_seed, n, cx.max_d, g.scale,
               cx.radius, cx.min_bits, grown);
    return GPK_OK;
}

// steps 4-5.  The join statistics, when on, count these candidates as gpk_dwithin_join counts its own (the n seed evaluations of step
// 2 are not candidates).  Scratch: 256 bytes of counters (word 0: listed candidates), the payload dist[n_cand] when distances were asked for, then
// the extra 8 (+ 4 for two non-point columns) bytes per candidate: dist[n_cand] for a call without a payload, the list [n_cand].
int32_t nearest_any_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit,
                           unsigned long long* stats, hipStream_t s) {
    const NaCtx& cx = *(const NaCtx*)ctx;
    char* p = (char*)scratch;
    uint32_t* n_large = (uint32_t*)p;
    p += 256;
    double* dist = (double*)p;  // (the payload when there is one, else the extra bytes' first array: the same place)
    p += sizeof(double) * (size_t)n_cand * (cx.p.payload_out ? 2 : 1);
    uint32_t* large = cx.pair_kernels ? (uint32_t*)p : nullptr;
    const RowCands cs{cand_l, cand_r, (int64_t)n_cand, cx.lbox, cx.rbox, cx.radius, hit, dist, stats, "gpk_nearest_any_refine",
                      "gpk_nearest_any_refine_large"};
    GPK_TRY(refine_row_candidates("nearest_join_any", cx.p.left, cx.p.right, cs, large, n_large, s));
    GPK_LAUNCH("gpk_nearest_any_min", nearest_any_min_kernel, per_element(n_cand), dim3(256), 0, s, cand_l, (const double*)dist,
               (const double*)cx.radius, (int64_t)n_cand, cx.min_bits);
    GPK_LAUNCH("gpk_nearest_any_hit", nearest_any_hit_kernel, per_element(n_cand), dim3(256), 0, s, cand_l, (const double*)dist,
               (const double*)cx.radius, (const unsigned long long*)cx.min_bits, (int64_t)n_cand, hit);
    return GPK_OK;
}

bool nearest_any_family(int32_t t) {
    return t == GPK_GEOM_POINT || t == GPK_GEOM_MULTIPOINT || t == GPK_GEOM_LINESTRING || t == GPK_GEOM_MULTILINESTRING || t == GPK_GEOM_POLYGON ||
           t == GPK_GEOM_MULTIPOLYGON;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_nearest_join_any(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double max_distance,
                                        uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist, int64_t pair_capacity,
                                        int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (!(max_distance >= 0.0))
        return fail(GPK_ERR_INVALID_ARGUMENT, "nearest_join_any: max_distance must be >= 0 (INFINITY: no limit), got %g", max_distance);
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    if (!nearest_any_family(left->d.type) || !nearest_any_family(right->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "nearest_join_any: unsupported geometry types %d, %d", left->d.type, right->d.type);
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "nearest_join_any"));
    NaCtx cx{};
    cx.p = PayloadCtx{left, right, "gpk_nearest_any_gather", sizeof(double), nullptr};
    cx.max_d = max_distance;
    cx.pair_kernels = left->d.type != GPK_GEOM_POINT && right->d.type != GPK_GEOM_POINT;
    const PayloadJoin join{"nearest_join_any", &cx.p, nearest_any_refine, sizeof(double) + (cx.pair_kernels ? sizeof(uint32_t) : 0), nearest_any_boxes};

    // the per-row state of the search lives in one block from the device cache (payload_join's arenas are carved by its own stages);
    // the empty cases never reach the hook
    const int64_t n = left->d.n_geoms;
    char* block = nullptr;
    if (n > 0 && n <= (int64_t)INT32_MAX && right->d.n_geoms > 0) {
        GPK_TRY(require_device());
        const size_t f64 = align256(sizeof(double) * (size_t)n), u32 = align256(sizeof(uint32_t) * (size_t)n);
        const hipError_t e = cached_malloc((void**)&block, 4 * f64 + 3 * u32 + align256((size_t)n) + 256);
        if (e != hipSuccess) return fail(GPK_ERR_OOM, "nearest_join_any: %s", hipGetErrorString(e));
        char* p = block;
        cx.radius = (double*)p, p += f64;
        cx.u_seed = (double*)p, p += f64;
        cx.t_seed = (double*)p, p += f64;
        cx.min_bits = (unsigned long long*)p, p += f64;
        cx.seed_l = (uint32_t*)p, p += u32;
        cx.seed_r = (uint32_t*)p, p += u32;
        cx.seed_large = (uint32_t*)p, p += u32;
        cx.seed_hit = (uint8_t*)p, p += align256((size_t)n);
        cx.seed_n_large = (uint32_t*)p;
    }
    const int32_t rc = payload_join(join, right_index, left_row_base, out_counts, out_pairs, out_dist, pair_capacity, n_pairs, out_space, stream);
    if (block) {
        (void)hipStreamSynchronize((hipStream_t)stream);  // (an error return may leave kernels that read the block in flight)
        cached_free(block);
    }
    return rc;
}
