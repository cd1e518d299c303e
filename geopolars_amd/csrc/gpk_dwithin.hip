// gpk_dwithin.hip — within-distance join (GeoPandas sjoin(predicate="dwithin", distance=d)) and row-wise dwithin for every pair of
// POINT, MULTIPOINT, LINESTRING, MULTILINESTRING, POLYGON and MULTIPOLYGON columns.  Contract: include/geopolars_hip.h
// (gpk_dwithin_join, gpk_dwithin_rowwise).
//
// Pipeline of the join (one for all 36 ordered pairs):
//   1. left boxes (gpk_bounds) grown on every side by g = distance + margin (dwithin_grow_kernel);
//   2. candidates: the staged bbox candidate generator of gpk_bboxjoin.hip (gpk_candjoin.h) with the grown boxes in the left boxes' place —
//      every (l, r) whose right box meets the grown left box, once, ordered by (l, r);
//   3. refine, G lanes per CANDIDATE (the unit of parallelism is the candidate, not the left row: ragged candidate lists do not
//      unbalance waves): first the distance between the two UNGROWN boxes — above distance + margin the candidate is rejected before a
//      coordinate is read, which settles most candidates of a grown-box search — then the exact distance d and hit = d <= distance:
//        a POINT on either side   point_geom_distance<G, KIND> of the other side, G = distance_group_size(other side)
//        two non-point sides      pair_distance_group<G, KA, KB> (gpk_pairdist.h), G = pairdist_group_size; a candidate with
//                                 n_A * n_B > PD_LARGE_COST is appended to a list and finished by pair_distance_workgroup in a second
//                                 launch whose fixed grid reads the list's length on the device
//      These are the routines, group sizes and lane orders of gpk_distance_rowwise's per-row kernels, so d is bit for bit the double
//      that call returns for the pair, and the pair test is a comparison of that double with `distance`.
//   4. emit: the generator's count / scan / emit of the hits, plus a gather of the hits' distances for out_dist.
// Steps 2 and 4 and the host work around them (temporary index, arenas, copies) are payload_join (gpk_candjoin.h); this file brings the
// grown boxes (dwithin_boxes) and the refine.
//
// Margin.  The candidate set must contain every pair whose COMPUTED distance is <= distance although boxes, cell function and distances
// are rounded.  Let D be the exact distance of a pair and d the computed one: |d - D| <= 16 u (D + 2 lmax) (the distance routines'
// a-priori bound; lmax = the pair's longest segment, at most the larger box's width + height).  The boxes are exact (minima and maxima
// of coordinates), and the gap between them along either axis is at most D.  So d <= distance implies gap <= distance + 16 u (distance
// + 2 lmax) (1 + O(u)).  The grown box is computed as fl(max + g) >= (max + g)(1 - u), g = fl(distance + m): the right box's edge, which
// lies within the grid's extent, is reached when m exceeds 16 u (distance + 2 lmax) + u (|max| + g) + the rounding of g.  With
//   m = 64 eps (|x0| + |y0| + extent width + extent height + |minx| + |miny| + |maxx| + |maxy| + distance),   eps = 2u,
// every term is covered several times over: lmax of the right row <= the extent, lmax of the left row <= |minx| + ... + |maxy|.  The
// candidate generator then compares the grown box with the right boxes and assigns cells with the monotone cell function the directory
// was built with, exactly: nothing is lost there (its dedupe rule holds for any left box).  The refine's box test uses the same form of
// margin with both boxes' coordinates in the grid's place.  A margin only ever costs a few extra exact evaluations.
#include <cfloat>
#include <cmath>

#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_distance.h"
#include "gpk_dwithin_refine.h"
#include "gpk_pairdist.h"

namespace gpk {

namespace {

__global__ __launch_bounds__(256) void dwithin_grow_kernel(const double4* __restrict__ in, int64_t n, double distance, double scale,
                                                           double4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double4 b = in[i];
    const double m = 64.0 * DBL_EPSILON * (scale + fabs(b.x) + fabs(b.y) + fabs(b.z) + fabs(b.w) + distance);
    const double g = distance + m;
    out[i] = make_double4(b.x - g, b.y - g, b.z + g, b.w + g);  // (an empty row's NaN box stays NaN: no candidates)
}

// Can the pair lie within t?  The distance between the two (exact) boxes against t plus the margin; false when a box has a NaN.
// Null rows never reach the refine: every candidate kernel of gpk_bboxjoin.hip (bbox_cand_stage_kernel, cand_compact_kernel, bbox_cand_kernel)
// tests the validity bit of the left and of the right row before it lists a pair, whatever the rows' boxes hold, so the refine kernels
// read (l, r) without a validity test of their own (one in the point kernels cost 15 % of the C3 refine: 350 against 304 ms).
__device__ __forceinline__ bool boxes_within(const double4 a, const double4 b, double t) {
    const double dx = fmax(fmax(b.x - a.z, a.x - b.z), 0.0), dy = fmax(fmax(b.y - a.w, a.y - b.w), 0.0);
    const double m = 64.0 * DBL_EPSILON * (fabs(a.x) + fabs(a.y) + fabs(a.z) + fabs(a.w) + fabs(b.x) + fabs(b.y) + fabs(b.z) + fabs(b.w) + t);
    return sqrt(dx * dx + dy * dy) <= t + m;  // (m is NaN when a coordinate is: the comparison fails)
}

// does row j of a non-point column hold a coordinate (empty members of a multi-geometry are ignored)
template <int KIND>
__device__ __forceinline__ bool has_coordinate(const DevGeo& g, int64_t j) {
    const RowSeqs r = row_seqs<KIND>(g, j);
    return r.c1 > r.c0;
}
__device__ __forceinline__ bool has_coordinate_any(const DevGeo& g, int64_t j) {
    switch (g.type) {
    case GPK_GEOM_POINT: {
        const double2 p = g.xy[j];
        return !isnan(p.x) && !isnan(p.y);
    }
    case GPK_GEOM_MULTIPOINT: return has_coordinate<GPK_GEOM_MULTIPOINT>(g, j);
    case GPK_GEOM_LINESTRING: return has_coordinate<GPK_GEOM_LINESTRING>(g, j);
    case GPK_GEOM_MULTILINESTRING: return has_coordinate<GPK_GEOM_MULTILINESTRING>(g, j);
    case GPK_GEOM_POLYGON: return has_coordinate<GPK_GEOM_POLYGON>(g, j);
    default: return has_coordinate<GPK_GEOM_MULTIPOLYGON>(g, j);
    }
}

struct Cands {
    const uint32_t* l;
    const uint32_t* r;
    int64_t n;
    const double4* lbox;  // the left rows' own boxes (not grown)
    const double4* rbox;  // the index's boxes of the right rows
    double t;
    uint8_t* hit;
    double* dist;                // per candidate, or nullptr
    unsigned long long* stats;   // join statistics words or nullptr: [2] += candidates, [3] += candidates the box test rejected
};

// The refine kernels take the candidates as `Cands` (one threshold: gpk_dwithin_join, whose kernels read it as the scalar it always was)
// or as `RowCands` (gpk_dwithin_refine.h: a threshold per LEFT row, gpk_nearest_join_any's search radius).
__device__ __forceinline__ double threshold_of(const Cands& cs, int64_t) { return cs.t; }
__device__ __forceinline__ double threshold_of(const RowCands& cs, int64_t l) { return cs.t[l]; }

template <class CS>
__device__ __forceinline__ void count_stats(const CS& cs, unsigned long long rejected, int lane) {
    if (!cs.stats) return;
    if (lane == 0 && rejected) atomicAdd(cs.stats + 3, rejected);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(cs.stats + 2, (unsigned long long)cs.n);
}

// A POINT column on one side (both: KIND == POINT, G == 1): G lanes per candidate.  `point_left`: pts is the caller's left column.
template <int G, int KIND, class CS>
__global__ __launch_bounds__(256) void dwithin_point_refine_kernel(DevGeo pts, DevGeo other, bool point_left, CS cs) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    unsigned long long rejected = 0;
    for (int64_t c = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; c < cs.n; c += groups) {
        const int64_t l = cs.l[c], r = cs.r[c];
        const int64_t ip = point_left ? l : r, jo = point_left ? r : l;
        const double t = threshold_of(cs, l);
        double d = NAN;
        if (!boxes_within(cs.lbox[l], cs.rbox[r], t)) {
            ++rejected;
        } else {
            const double2 p = pts.xy[ip];
            bool ok = !isnan(p.x) && !isnan(p.y);
            // (the point routines give 0.0 for an empty row.  With boxes from gpk_bounds and the index an empty row has a NaN box and never
            // gets here; the test keeps the never-matched rule from resting on that alone.  The row-wise kernel below needs it.)
            if constexpr (KIND != GPK_GEOM_POINT) ok = ok && has_coordinate<KIND>(other, jo);
            if (ok) d = point_geom_distance<G, KIND>(other, jo, p.x, p.y, lane);
        }
        if (lane == 0) {
            cs.hit[c] = d <= t ? 1 : 0;
            if (cs.dist) cs.dist[c] = d;
        }
    }
    count_stats(cs, rejected, lane);
}

// Two non-point columns in canonical order (KA <= KB); `swapped`: gb is the caller's left column.  G lanes per candidate; candidates
// above PD_LARGE_COST are listed for dwithin_pair_large_kernel.
template <int G, int KA, int KB, class CS>
__global__ __launch_bounds__(256) void dwithin_pair_refine_kernel(DevGeo ga, DevGeo gb, bool swapped, CS cs, uint32_t* __restrict__ large,
                                                                  uint32_t* __restrict__ n_large) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    unsigned long long rejected = 0;
    for (int64_t c = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; c < cs.n; c += groups) {
        const int64_t l = cs.l[c], r = cs.r[c];
        const int64_t ia = swapped ? r : l, ib = swapped ? l : r;
        const double t = threshold_of(cs, l);
        double d = NAN;
        if (!boxes_within(cs.lbox[l], cs.rbox[r], t)) {
            ++rejected;
        } else {
            const RowSeqs a = row_seqs<KA>(ga, ia), b = row_seqs<KB>(gb, ib);
            const int na = a.c1 - a.c0, nb = b.c1 - b.c0;
            if (na > 0 && nb > 0) {
                if ((int64_t)na * nb > PD_LARGE_COST) {
                    if (lane == 0) large[atomicAdd(n_large, 1u)] = (uint32_t)c;
                    continue;
                }
                d = pair_distance_group<G, KA, KB>(ga, ia, a, gb, ib, b, lane);
            }
        }
        if (lane == 0) {
            cs.hit[c] = d <= t ? 1 : 0;
            if (cs.dist) cs.dist[c] = d;
        }
    }
    count_stats(cs, rejected, lane);
}

// One 256-lane work-group per listed candidate (pair_distance_workgroup: the routine of pairdist_large_kernel).
template <int KA, int KB, class CS>
__global__ __launch_bounds__(256) void dwithin_pair_large_kernel(DevGeo ga, DevGeo gb, bool swapped, CS cs, const uint32_t* __restrict__ large,
                                                                 const uint32_t* __restrict__ n_large) {
    __shared__ PairLargeLds lds;
    const uint32_t count = *n_large;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const int64_t c = large[e];
        const int64_t l = cs.l[c], r = cs.r[c];
        const double d = pair_distance_workgroup<KA, KB>(ga, swapped ? r : l, gb, swapped ? l : r, lds);
        if (threadIdx.x == 0) {
            cs.hit[c] = d <= threshold_of(cs, l) ? 1 : 0;
            if (cs.dist) cs.dist[c] = d;
        }
    }
}

// row-wise: the distance kernels' answer against the threshold; null, out-of-range, empty and NaN-point rows never match
__global__ __launch_bounds__(256) void dwithin_threshold_kernel(DevGeo a, DevGeo b, const uint32_t* __restrict__ rows, const double* __restrict__ d,
                                                                double t, int64_t n, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t j = rows ? (int64_t)rows[i] : i;
    const bool ok = dev::row_ok(a, i) && dev::row_ok(b, j) && has_coordinate_any(a, i) && has_coordinate_any(b, j);
    out[i] = ok && d[i] <= t ? 1 : 0;
}

struct DwCtx {
    PayloadCtx p;  // (p.payload_out: the distances were asked for)
    double t;
    bool pair_kernels;
    const double4 *lbox, *rbox;  // set by dwithin_boxes
};
// scratch of a call: 256 bytes of counters (word 0: listed candidates), then dist[n_cand] (when asked for), then the list [n_cand]
struct DwScratch {
    uint32_t* n_large;
    double* dist;
    uint32_t* large;
};
DwScratch carve(const DwCtx& cx, void* scratch, int64_t n_cand) {
    char* p = (char*)scratch;
    DwScratch sc;
    sc.n_large = (uint32_t*)p;
    p += 256;
    sc.dist = cx.p.payload_out ? (double*)p : nullptr;
    if (cx.p.payload_out) p += sizeof(double) * (size_t)n_cand;
    sc.large = cx.pair_kernels ? (uint32_t*)p : nullptr;
    return sc;
}

// the profile stages of the two launches
inline const char* refine_label(const Cands&) { return "gpk_dwithin_refine"; }
inline const char* refine_label(const RowCands& cs) { return cs.label; }
inline const char* large_label(const Cands&) { return "gpk_dwithin_refine_large"; }
inline const char* large_label(const RowCands& cs) { return cs.label_large; }

template <int KIND, class CS>
int32_t launch_point_refine(int G, const DevGeo& pts, const DevGeo& other, bool point_left, const CS& cs, hipStream_t s) {
    const dim3 grid = group_grid(cs.n, G);
    if (G == 1)
        GPK_LAUNCH(refine_label(cs), (dwithin_point_refine_kernel<1, KIND, CS>), grid, dim3(256), 0, s, pts, other, point_left, cs);
    else if (G == 8)
        GPK_LAUNCH(refine_label(cs), (dwithin_point_refine_kernel<8, KIND, CS>), grid, dim3(256), 0, s, pts, other, point_left, cs);
    else
        GPK_LAUNCH(refine_label(cs), (dwithin_point_refine_kernel<32, KIND, CS>), grid, dim3(256), 0, s, pts, other, point_left, cs);
    return GPK_OK;
}

template <int KA, int KB, class CS>
int32_t launch_pair_refine(const DevGeo& ga, const DevGeo& gb, bool swapped, const CS& cs, uint32_t* large, uint32_t* n_large, hipStream_t s) {
    const int G = pairdist_group_size(ga, gb);
    const dim3 grid = group_grid(cs.n, G);
    if (G == 8)
        GPK_LAUNCH(refine_label(cs), (dwithin_pair_refine_kernel<8, KA, KB, CS>), grid, dim3(256), 0, s, ga, gb, swapped, cs, large, n_large);
    else
        GPK_LAUNCH(refine_label(cs), (dwithin_pair_refine_kernel<32, KA, KB, CS>), grid, dim3(256), 0, s, ga, gb, swapped, cs, large, n_large);
    // the listed candidates: a fixed grid that reads the list's length on the device (idle work-groups return at once)
    const int64_t lb = (int64_t)cu_count() * 4 < cs.n ? (int64_t)cu_count() * 4 : cs.n;
    GPK_LAUNCH(large_label(cs), (dwithin_pair_large_kernel<KA, KB, CS>), dim3((unsigned)lb), dim3(256), 0, s, ga, gb, swapped, cs,
               (const uint32_t*)large, (const uint32_t*)n_large);
    return GPK_OK;
}

// The exact distance of every candidate of `cs` (and hit = d <= its threshold) for the columns L (the candidates' l) and R (their r);
// `large` (cs.n entries) and `n_large` (one word, zeroed here) are read only when neither column is POINT.
template <class CS>
int32_t refine_candidates(const char* who, const DevGeo& L, const DevGeo& R, const CS& cs, uint32_t* large, uint32_t* n_large, hipStream_t s) {
    if (L.type == GPK_GEOM_POINT || R.type == GPK_GEOM_POINT) {
        // the POINT column takes the point's place (the left one when both are), as in gpk_distance_rowwise
        const bool point_left = L.type == GPK_GEOM_POINT;
        const DevGeo &pts = point_left ? L : R, &other = point_left ? R : L;
        const int G = distance_group_size(other);
        switch (other.type) {
        case GPK_GEOM_POINT: return launch_point_refine<GPK_GEOM_POINT>(1, pts, other, point_left, cs, s);
        case GPK_GEOM_MULTIPOINT: return launch_point_refine<GPK_GEOM_MULTIPOINT>(G, pts, other, point_left, cs, s);
        case GPK_GEOM_LINESTRING: return launch_point_refine<GPK_GEOM_LINESTRING>(G, pts, other, point_left, cs, s);
        case GPK_GEOM_MULTILINESTRING: return launch_point_refine<GPK_GEOM_MULTILINESTRING>(G, pts, other, point_left, cs, s);
        case GPK_GEOM_POLYGON: return launch_point_refine<GPK_GEOM_POLYGON>(G, pts, other, point_left, cs, s);
        default: return launch_point_refine<GPK_GEOM_MULTIPOLYGON>(G, pts, other, point_left, cs, s);
        }
    }
    GPK_HIP(hipMemsetAsync(n_large, 0, sizeof(uint32_t), s));
    const bool swapped = L.type > R.type;
    const DevGeo& ga = swapped ? R : L;
    const DevGeo& gb = swapped ? L : R;
    constexpr int MP = GPK_GEOM_MULTIPOINT, LS = GPK_GEOM_LINESTRING, MLS = GPK_GEOM_MULTILINESTRING, PG = GPK_GEOM_POLYGON,
                  MPG = GPK_GEOM_MULTIPOLYGON;
#define PD(KA, KB) \
    if (ga.type == KA && gb.type == KB) return launch_pair_refine<KA, KB>(ga, gb, swapped, cs, large, n_large, s)
    PD(LS, LS); PD(LS, PG); PD(LS, MP); PD(LS, MLS); PD(LS, MPG);
    PD(PG, PG); PD(PG, MP); PD(PG, MLS); PD(PG, MPG);
    PD(MP, MP); PD(MP, MLS); PD(MP, MPG);
    PD(MLS, MLS); PD(MLS, MPG);
    PD(MPG, MPG);
#undef PD
    return fail(GPK_ERR_MISMATCHED_GEOMETRY, "%s: no kernel for geometry types %d, %d", who, L.type, R.type);
}

int32_t dwithin_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit,
                       unsigned long long* stats, hipStream_t s) {
    const DwCtx& cx = *(const DwCtx*)ctx;
    const DwScratch sc = carve(cx, scratch, n_cand);
    const Cands cs{cand_l, cand_r, (int64_t)n_cand, cx.lbox, cx.rbox, cx.t, hit, sc.dist, stats};
    return refine_candidates("dwithin_join", cx.p.left->d, cx.p.right->d, cs, sc.large, sc.n_large, s);
}

// the left boxes of the candidate search: the rows' own boxes grown by the distance and the margin (see the top of the file)
int32_t dwithin_boxes(PayloadCtx* ctx, const gpk_index* right_index, const double4* own, double4* grown, int64_t n, hipStream_t s) {
    DwCtx& cx = *(DwCtx*)ctx;
    cx.lbox = own;
    cx.rbox = right_index->v.bbox;
    // the magnitude the margin scales with: the directory's origin and extent (an axis of zero extent has inv = 0: one column / row)
    const GridParams& h = right_index->host_grid;
    const double scale = fabs(h.x0) + fabs(h.y0) + (h.inv_w > 0.0 ? (double)h.gx / h.inv_w : 0.0) + (h.inv_h > 0.0 ? (double)h.gy / h.inv_h : 0.0);
    GPK_LAUNCH("gpk_dwithin_grow", dwithin_grow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, own, n, cx.t, scale, grown);
    return GPK_OK;
}

bool dwithin_family(int32_t t) {
    return t == GPK_GEOM_POINT || t == GPK_GEOM_MULTIPOINT || t == GPK_GEOM_LINESTRING || t == GPK_GEOM_MULTILINESTRING || t == GPK_GEOM_POLYGON ||
           t == GPK_GEOM_MULTIPOLYGON;
}

}  // namespace

int32_t refine_row_candidates(const char* who, const gpk_geoarray* left, const gpk_geoarray* right, const RowCands& cs, uint32_t* large,
                              uint32_t* n_large, hipStream_t s) {
    return refine_candidates(who, left->d, right->d, cs, large, n_large, s);
}

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_dwithin_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double distance,
                                    uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist, int64_t pair_capacity,
                                    int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (!(distance >= 0.0) || std::isinf(distance))
        return fail(GPK_ERR_INVALID_ARGUMENT, "dwithin_join: distance must be finite and >= 0, got %g", distance);
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    if (!dwithin_family(left->d.type) || !dwithin_family(right->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "dwithin_join: unsupported geometry types %d, %d", left->d.type, right->d.type);
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "dwithin_join"));
    DwCtx cx{{left, right, "gpk_dwithin_gather", sizeof(double), nullptr}, distance,
             left->d.type != GPK_GEOM_POINT && right->d.type != GPK_GEOM_POINT, nullptr, nullptr};
    const PayloadJoin join{"dwithin_join", &cx.p, dwithin_refine, cx.pair_kernels ? sizeof(uint32_t) : 0, dwithin_boxes};
    return payload_join(join, right_index, left_row_base, out_counts, out_pairs, out_dist, pair_capacity, n_pairs, out_space, stream);
}

extern "C" int32_t gpk_dwithin_rowwise(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double distance, uint8_t* out,
                                       int32_t out_space, void* stream) {
    if (!a || !b || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(distance >= 0.0) || std::isinf(distance))
        return fail(GPK_ERR_INVALID_ARGUMENT, "dwithin: distance must be finite and >= 0, got %g", distance);
    if (!dwithin_family(a->d.type) || !dwithin_family(b->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "dwithin: unsupported geometry types %d, %d", a->d.type, b->d.type);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = a->d.n_geoms;
    if (!b_rows && n != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "dwithin: row counts differ (%lld vs %lld)", (long long)n, (long long)b->d.n_geoms);
    if (b_rows && a->d.type != GPK_GEOM_POINT && b->d.type == GPK_GEOM_POINT)
        return fail(GPK_ERR_INVALID_ARGUMENT, "dwithin: b_rows requires the POINT array on the left");
    if (n == 0) return GPK_OK;
    // (the distance call carves workspace() itself; this call's buffers live in an auxiliary arena)
    Scratch sc(workspace_aux(0));
    double* d;
    const uint32_t* rows_dev;
    uint8_t* out_dev;
    sc.add(d, (size_t)n);
    sc.stage_in(rows_dev, b_rows, out_space, (size_t)n);
    sc.stage(out_dev, out, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    GPK_TRY(gpk_distance_rowwise(a, b, rows_dev, d, GPK_MEM_DEVICE, stream));
    GPK_LAUNCH("gpk_dwithin_threshold", dwithin_threshold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a->d, b->d, rows_dev,
               (const double*)d, distance, n, out_dev);
    return sc.copy_back(s);
}
