// gpk_bboxjoin.hip — the staged box-candidate join: candidates per left box from the right side's grid directory, the caller's refine
// (CandRefine, gpk_candjoin.h), then count / scan / emit of the hits sorted by (l, r); and payload_join, the driver of the joins that
// return a value per pair over it (temporary index, boxes, payload staging and the one gather kernel).
//
//   candidates  == intersection_candidates_with_other_tree            spatial_index.rs:74-76
//   the refines of gpk_spatial_join's polygonal and lineal arms       spatial_index.rs:83-143
//   gpk_index_query_envelope == locate_in_envelope(_intersecting)     spatial_index.rs:385-387,424-426
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "gpk_device.h"
#include "gpk_index.h"
#include "gpk_candjoin.h"
#include "gpk_polypoly.h"
#include "gpk_contains.h"
#include "gpk_lineal.h"
#include "gpk_scan.h"

namespace gpk {

// ================================= polygonal x polygonal join ======================================
// Candidate generation of spatial_index.rs:74-76 for bbox-shaped left rows: every directory cell the left
// bbox touches is visited; a pair seen in several cells is processed only in the cell that holds the lower
// left corner of the two boxes' intersection (computed with the same monotone cell function, so that cell
// is in both registration ranges).  The exact refine is Intersects<Polygon> (gpk_polypoly.h).
template <typename F>
__device__ __forceinline__ void for_each_bbox_candidate(const IndexView& ix, const GridParams& g, const double4 lb, F&& f) {
    if (!(lb.x == lb.x)) return;  // empty left geometry
    const int cx0 = dev::cell_of(lb.x, g.x0, g.inv_w, g.gx), cx1 = dev::cell_of(lb.z, g.x0, g.inv_w, g.gx);
    const int cy0 = dev::cell_of(lb.y, g.y0, g.inv_h, g.gy), cy1 = dev::cell_of(lb.w, g.y0, g.inv_h, g.gy);
    for (int cy = cy0; cy <= cy1; ++cy)
        for (int cx = cx0; cx <= cx1; ++cx) {
            const int c = cy * g.gx + cx;
            auto visit = [&](int j, const double4 rb) {
                if (lb.z < rb.x || lb.w < rb.y || rb.z < lb.x || rb.w < lb.y) return;  // closed-interval overlap test
                const double rx = lb.x > rb.x ? lb.x : rb.x, ry = lb.y > rb.y ? lb.y : rb.y;
                if (dev::cell_of(rx, g.x0, g.inv_w, g.gx) != cx || dev::cell_of(ry, g.y0, g.inv_h, g.gy) != cy) return;
                f(j);
            };
            const int k1 = ix.cell_off[c + 1];
            for (int k = ix.cell_off[c]; k < k1; k += 2) {  // two items per trip: both ids, then both boxes, in flight together
                const bool two = k + 1 < k1;
                const int j0 = ix.items[k], j1 = ix.items[two ? k + 1 : k];
                const double4 b0 = ix.bbox[j0], b1 = ix.bbox[j1];
                visit(j0, b0);
                if (two) visit(j1, b1);
            }
        }
}

// Stage 1: candidates.  One lane per left row lists the right rows whose closed bbox overlaps the row's bbox
// (count pass, then fill pass into the row's slice, sorted by right id: the hits then come out sorted).  Rows with a
// handful of candidates sort their slice in place; a row with more than CAND_INLINE_SORT (one country against a
// column of parcels) raises *big_rows in the count pass and every slice goes through one segmented radix sort instead.
constexpr int CAND_INLINE_SORT = 48;
template <bool WRITE>
__global__ __launch_bounds__(256) void bbox_cand_kernel(DevGeo left, DevGeo right, IndexView ix, const double4* __restrict__ lbbox,
                                                         int32_t* __restrict__ cand_cnt, const int32_t* __restrict__ cand_off,
                                                         uint32_t* __restrict__ cand_r, uint32_t* __restrict__ cand_l,
                                                         int32_t* __restrict__ big_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= left.n_geoms) return;
    int cnt = 0;
    const int64_t o0 = WRITE ? (int64_t)cand_off[i] : 0;
    if (dev::valid_row(left.validity, i)) {
        const GridParams g = *ix.grid;
        for_each_bbox_candidate(ix, g, lbbox[i], [&](int j) {
            if (!dev::valid_row(right.validity, j)) return;
            if (WRITE) cand_r[o0 + cnt] = (uint32_t)j;
            ++cnt;
        });
    }
    if (!WRITE) {
        cand_cnt[i] = cnt;
        if (cnt > CAND_INLINE_SORT) *big_rows = 1;
        return;
    }
    for (int a = 1; a < cnt && cnt <= CAND_INLINE_SORT; ++a) {  // rows have a handful of candidates
        const uint32_t key = cand_r[o0 + a];
        int b = a - 1;
        while (b >= 0 && cand_r[o0 + b] > key) {
            cand_r[o0 + b + 1] = cand_r[o0 + b];
            --b;
        }
        cand_r[o0 + b + 1] = key;
    }
    for (int a = 0; a < cnt; ++a) cand_l[o0 + a] = (uint32_t)i;  // left row of every candidate: the refine reads it directly
}

// One search instead of two for ordinary rows: the count pass also leaves each row's first CAND_STAGE candidates (sorted) in a padded
// staging slice; when no row has more (nearly every join: rows have a handful), cand_compact_kernel moves the slices to their scanned
// offsets and the second directory walk (bbox_cand_kernel<true>: 0.90 ms of the 6.1 ms C4 join) does not run.
constexpr int CAND_STAGE = 16;
static_assert(CAND_STAGE <= CAND_INLINE_SORT, "a staged row is one that the fill pass would have sorted inline");
// Round 6: CAND_LANES lanes per left row.  One lane per row walked its cells' items as a chain of dependent requests — cell offsets, then
// ids two at a time, then their boxes — about eight round trips a row with the lanes of a wave on rows of different lengths (0.82 ms
// for the 1 M rows of C4); the lanes of a row now take the items of a cell side by side (ids together, boxes together: two round trips
// a cell) and append their finds to the row's slice with one ballot.
constexpr int CAND_LANES = 8;
__global__ __launch_bounds__(256) void bbox_cand_stage_kernel(DevGeo left, DevGeo right, IndexView ix, const double4* __restrict__ lbbox,
                                                               int32_t* __restrict__ cand_cnt, uint32_t* __restrict__ stage,
                                                               int32_t* __restrict__ flags /* [0]: big rows, [1]: rows beyond CAND_STAGE */) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t / CAND_LANES;
    const int sub = (int)(threadIdx.x & (CAND_LANES - 1)), gbase = (int)(threadIdx.x & 63) & ~(CAND_LANES - 1);
    if (i >= left.n_geoms) return;  // (whole groups: CAND_LANES divides the block)
    int cnt = 0;
    uint32_t* mine = stage + i * CAND_STAGE;
    const double4 lb = lbbox[i];
    if (dev::valid_row(left.validity, i) && lb.x == lb.x) {
        const GridParams g = *ix.grid;
        const int cx0 = dev::cell_of(lb.x, g.x0, g.inv_w, g.gx), cx1 = dev::cell_of(lb.z, g.x0, g.inv_w, g.gx);
        const int cy0 = dev::cell_of(lb.y, g.y0, g.inv_h, g.gy), cy1 = dev::cell_of(lb.w, g.y0, g.inv_h, g.gy);
        for (int cy = cy0; cy <= cy1; ++cy)
            for (int cx = cx0; cx <= cx1; ++cx) {
                const int c = cy * g.gx + cx;
                const int k0 = ix.cell_off[c], k1 = ix.cell_off[c + 1];
                for (int kb = k0; kb < k1; kb += CAND_LANES) {  // (group-uniform trip count)
                    const int k = kb + sub;
                    bool keep = false;
                    int j = 0;
                    if (k < k1) {
                        j = ix.items[k];
                        const double4 rb = ix.bbox[j];
                        // closed-interval overlap, and the pair belongs to THIS cell: the one that holds the lower-left corner of the two
                        // boxes' intersection (for_each_bbox_candidate)
                        if (!(lb.z < rb.x || lb.w < rb.y || rb.z < lb.x || rb.w < lb.y)) {
                            const double rx = lb.x > rb.x ? lb.x : rb.x, ry = lb.y > rb.y ? lb.y : rb.y;
                            keep = dev::cell_of(rx, g.x0, g.inv_w, g.gx) == cx && dev::cell_of(ry, g.y0, g.inv_h, g.gy) == cy && dev::valid_row(right.validity, j);
                        }
                    }
                    const uint32_t m = (uint32_t)((__ballot(keep) >> gbase) & ((1u << CAND_LANES) - 1u));
                    const int at = cnt + __popc(m & ((1u << sub) - 1u));
                    if (keep && at < CAND_STAGE) mine[at] = (uint32_t)j;  // (in directory order: cand_compact_kernel sorts the slice across its 16 lanes)
                    cnt += __popc(m);
                }
            }
    }
    if (sub == 0) {
        cand_cnt[i] = cnt;
        if (cnt > CAND_STAGE) flags[1] = 1;
        if (cnt > CAND_INLINE_SORT) flags[0] = 1;
    }
}
// (a row with more than CAND_STAGE candidates — a dense cluster — walks the directory again, like bbox_cand_kernel<true>: one lane of
// its CAND_STAGE; rows beyond CAND_INLINE_SORT send the whole join down the two-search path with its segmented sort)
__global__ __launch_bounds__(256) void cand_compact_kernel(DevGeo left, DevGeo right, IndexView ix, const double4* __restrict__ lbbox,
                                                            const int32_t* __restrict__ cand_cnt, const int32_t* __restrict__ cand_off,
                                                            const uint32_t* __restrict__ stage, uint32_t* __restrict__ cand_r,
                                                            uint32_t* __restrict__ cand_l) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t / CAND_STAGE;
    const int j = (int)(t % CAND_STAGE);
    if (i >= left.n_geoms) return;
    const int cnt = cand_cnt[i];
    const int64_t o0 = (int64_t)cand_off[i];
    if (cnt <= CAND_STAGE) {
        // the row's slice, sorted by right id across the row's CAND_STAGE lanes: a bitonic network of ten shuffle steps (the count
        // pass used to keep the slice sorted by insertion — a chain of dependent global loads per candidate)
        static_assert(CAND_STAGE == 16, "the sorting network below is written for 16 lanes per row");
        uint32_t v = j < cnt ? stage[t] : 0xFFFFFFFFu;
#pragma unroll
        for (int k = 2; k <= CAND_STAGE; k <<= 1) {
#pragma unroll
            for (int d = k >> 1; d > 0; d >>= 1) {
                const uint32_t w = __shfl_xor(v, d, CAND_STAGE);
                const bool keep_min = ((j & d) == 0) == ((j & k) == 0);
                v = keep_min ? (v < w ? v : w) : (v > w ? v : w);
            }
        }
        if (j < cnt) {
            cand_r[o0 + j] = v;
            cand_l[o0 + j] = (uint32_t)i;
        }
        return;
    }
    if (j != 0) return;
    int m = 0;
    const GridParams g = *ix.grid;
    for_each_bbox_candidate(ix, g, lbbox[i], [&](int r) {
        if (!dev::valid_row(right.validity, r)) return;
        int b = m - 1;  // insertion into the ascending prefix
        while (b >= 0 && cand_r[o0 + b] > (uint32_t)r) {
            cand_r[o0 + b + 1] = cand_r[o0 + b];
            --b;
        }
        cand_r[o0 + b + 1] = (uint32_t)r;
        ++m;
    });
    for (int a = 0; a < m; ++a) cand_l[o0 + a] = (uint32_t)i;
}

// Stage 2: exact refine, JOIN_GS lanes per candidate pair (pairs are independent: the unit of parallelism is the
// pair, not the row, so ragged candidate lists do not unbalance waves).
constexpr int JOIN_GS = 16;
__device__ __forceinline__ int64_t row_of_candidate(const int32_t* __restrict__ off, int64_t n_rows, int64_t c) {
    int64_t lo = 0, hi = n_rows;  // largest row with off[row] <= c
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= c)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
// (a minimum of four waves per SIMD — 128 registers instead of 141 — was 4 % faster, 4.06 -> 3.90 ms, and wrote 1.1 GB of spilled
// registers per launch to scratch memory, WRITE_SIZE 9.7 MB -> 1.14 GB: not taken)
__global__ __launch_bounds__(256, 1) void pair_refine_kernel(DevGeo left, DevGeo right, const uint32_t* __restrict__ cand_l,
                                                           const uint32_t* __restrict__ cand_r, int64_t n_cand,
                                                           const double4* __restrict__ lbbox, const double4* __restrict__ rbbox,
                                                           uint8_t* __restrict__ hit, bool l_one_ring, bool r_one_ring) {
    // (l_one_ring / r_one_ring: every polygon of that POLYGON column is known to have exactly one ring — ring r is geometry r)
    // per group: the staging slice of the small-pair path, which doubles as the two in-window segment lists of the general one
    static_assert(sizeof(PairSmallLds) >= 2 * PP_LIST * sizeof(double4), "the general routine's lists fit the small-pair slice");
    __shared__ PairSmallLds slices[256 / JOIN_GS];
    const int lane = threadIdx.x & (JOIN_GS - 1);
    PairSmallLds* slice = slices + threadIdx.x / JOIN_GS;
    const bool plain = left.type == GPK_GEOM_POLYGON && right.type == GPK_GEOM_POLYGON && lbbox && rbbox;  // (uniform)
    // A group takes a CONTIGUOUS run of candidates: they are ordered by left row, so consecutive ones mostly share it and its ring stays
    // staged (round 6; a group used to stride over the list, staging both rings of every pair)
    const int64_t groups = (int64_t)gridDim.x * (256 / JOIN_GS);
    const int64_t per = (n_cand + groups - 1) / groups, g_id = (int64_t)blockIdx.x * (256 / JOIN_GS) + threadIdx.x / JOIN_GS;
    const int64_t c_lo = g_id * per, c_hi = c_lo + per < n_cand ? c_lo + per : n_cand;
    int64_t staged_i = -1;  // the left row whose ring is in slice->a
    for (int64_t c = c_lo; c < c_hi; ++c) {
        const int64_t i = (int64_t)cand_l[c], j = (int64_t)cand_r[c];
        bool h;
        bool small = false;
        int ca = 0, na = 0, cb = 0, nb = 0;
        if (plain) {  // two single-ring polygons of at most PP_SMALL coordinates: the staged path (gpk_polypoly.h)
            int ra0 = (int)i, ra1 = (int)i + 1, rb0 = (int)j, rb1 = (int)j + 1;
            if (!l_one_ring) {
                ra0 = left.geom_off[i];
                ra1 = left.geom_off[i + 1];
            }
            if (!r_one_ring) {
                rb0 = right.geom_off[j];
                rb1 = right.geom_off[j + 1];
            }
            if (ra1 - ra0 == 1 && rb1 - rb0 == 1) {
                ca = left.ring_off[ra0];
                na = left.ring_off[ra0 + 1] - ca;
                cb = right.ring_off[rb0];
                nb = right.ring_off[rb0 + 1] - cb;
                small = na >= 1 && nb >= 1 && na <= PP_SMALL && nb <= PP_SMALL;
            }
        }
        if (small) {
            h = polygon_pair_small<JOIN_GS>(left.xy + ca, na, right.xy + cb, nb, lbbox[i], rbbox[j], lane, slice, staged_i == i);
            staged_i = i;
        } else {
            h = polygonal_intersects_polygonal_group<JOIN_GS>(left, i, right, j, lane, reinterpret_cast<double4*>(slice), lbbox, rbbox);
            staged_i = -1;  // (the general routine keeps its segment lists in the slice)
        }
        if (lane == 0) hit[c] = h;
    }
}

// Contains<Polygon> for Polygon / MultiPolygon (spatial_index.rs:99-101,107-111; gpk_contains.h): the right polygon can only
// lie in a left geometry whose box holds its box, which settles most candidates of the (closed-overlap) candidate list.
__global__ __launch_bounds__(256) void pair_contains_kernel(DevGeo left, DevGeo right, const uint32_t* __restrict__ cand_l,
                                                             const uint32_t* __restrict__ cand_r, int64_t n_cand,
                                                             const double4* __restrict__ lbbox, const double4* __restrict__ rbbox,
                                                             uint8_t* __restrict__ hit) {
    const int lane = threadIdx.x & (JOIN_GS - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / JOIN_GS);
    for (int64_t c = (int64_t)blockIdx.x * (256 / JOIN_GS) + threadIdx.x / JOIN_GS; c < n_cand; c += groups) {
        const int64_t i = (int64_t)cand_l[c], j = (int64_t)cand_r[c];
        const double4 lb = lbbox[i], rb = rbbox[j];
        bool h = false;
        if (rb.x >= lb.x && rb.y >= lb.y && rb.z <= lb.z && rb.w <= lb.w) h = cont::polygonal_contains_polygonal_group<JOIN_GS>(left, i, right, j, lane);
        if (lane == 0) hit[c] = h;
    }
}

__global__ __launch_bounds__(256) void lineal_point_refine_kernel(DevGeo left, DevGeo right, const uint32_t* __restrict__ cand_l,
                                                                   const uint32_t* __restrict__ cand_r, int64_t n_cand,
                                                                   uint8_t* __restrict__ hit) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const int64_t i = cand_l[c], j = cand_r[c];
    const bool point_left = left.type == GPK_GEOM_POINT;
    const double2 p = point_left ? left.xy[i] : right.xy[j];
    bool h = false;
    if (p.x == p.x && p.y == p.y) h = point_left ? lineal_contains_point(right, j, p.x, p.y) : lineal_contains_point(left, i, p.x, p.y);
    hit[c] = h;
}

// Stage 3: per-row hit counts, then (after a scan) the (l, r) pairs in candidate order == sorted by (l, r).
template <bool WRITE>
__global__ __launch_bounds__(256) void pair_emit_kernel(int64_t n_rows, const int32_t* __restrict__ cand_off,
                                                         const uint32_t* __restrict__ cand_r, const uint8_t* __restrict__ hit,
                                                         int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
                                                         uint32_t left_base, uint2* __restrict__ pairs, int64_t capacity) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    int cnt = 0;
    const int64_t o0 = WRITE ? (int64_t)offsets[i] : 0;
    for (int c = cand_off[i]; c < cand_off[i + 1]; ++c) {
        if (!hit[c]) continue;
        if (WRITE && o0 + cnt < capacity) pairs[o0 + cnt] = make_uint2(left_base + (uint32_t)i, cand_r[c]);
        ++cnt;
    }
    if (!WRITE) counts[i] = cnt;
}

// payload_join: the per-candidate elements of row i's hits, in candidate order, at the row's offset of the output
namespace {
template <typename T>
__global__ __launch_bounds__(256) void payload_gather_kernel(int64_t n_rows, const int32_t* __restrict__ cand_off, const uint8_t* __restrict__ hit,
                                                             const int32_t* __restrict__ offsets, const T* __restrict__ payload,
                                                             T* __restrict__ out, int64_t capacity) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    int64_t o = offsets[i];
    for (int c = cand_off[i]; c < cand_off[i + 1]; ++c) {
        if (!hit[c]) continue;
        if (o < capacity) out[o] = payload[c];
        ++o;
    }
}
}  // namespace

__global__ void i32_to_u32_copy_kernel(const int32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)in[i];
}

// gpk_index_query_envelope's refine (rstar's locate_in_envelope_intersecting / locate_in_envelope, spatial_index.rs:385-387,424-426): a
// candidate's box already meets the query box (closed intervals: for_each_bbox_candidate); `contained` additionally asks that it lies
// inside it, bounds included (rstar AABB::contains_envelope)
__global__ __launch_bounds__(256) void query_boxes_kernel(const double4* __restrict__ in, int64_t n, double4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double4 b = in[i];
    const bool nan = !(b.x == b.x && b.y == b.y && b.z == b.z && b.w == b.w);
    out[i] = nan ? make_double4(NAN, NAN, NAN, NAN) : make_double4(fmin(b.x, b.z), fmin(b.y, b.w), fmax(b.x, b.z), fmax(b.y, b.w));
}
__global__ __launch_bounds__(256) void envelope_refine_kernel(const uint32_t* __restrict__ cand_l, const uint32_t* __restrict__ cand_r, int64_t n,
                                                               const double4* __restrict__ lbbox, const double4* __restrict__ rbbox, int contained,
                                                               uint8_t* __restrict__ hit) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double4 lb = lbbox[cand_l[i]], rb = rbbox[cand_r[i]];
    bool ok = rb.x == rb.x && lb.x == lb.x;
    if (contained) ok = ok && rb.x >= lb.x && rb.z <= lb.z && rb.y >= lb.y && rb.w <= lb.w;
    hit[i] = ok ? 1 : 0;
}

// ================================= host driver ================================================
// The refines of gpk_spatial_join and gpk_index_query_envelope as CandRefine values (gpk_candjoin.h): one launch each.
static dim3 pair_group_grid(int32_t n_cand) {  // JOIN_GS lanes per candidate, at most 64 work-groups a compute unit
    int64_t blocks = ((int64_t)n_cand + (256 / JOIN_GS) - 1) / (256 / JOIN_GS);
    const int64_t cap = (int64_t)cu_count() * 64;
    if (blocks > cap) blocks = cap;
    return dim3((unsigned)blocks);
}
static int32_t refine_polygonal_intersects(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void*, uint8_t* hit,
                                           unsigned long long*, hipStream_t s) {
    const BoxRefineCtx& cx = *(const BoxRefineCtx*)ctx;
    GPK_LAUNCH("gpk_pair_refine", pair_refine_kernel, pair_group_grid(n_cand), dim3(256), 0, s, cx.left->d, cx.right->d, cand_l, cand_r,
               (int64_t)n_cand, cx.lbbox, cx.rbbox, hit, cx.l_one_ring, cx.r_one_ring);
    return GPK_OK;
}
static int32_t refine_polygonal_contains(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void*, uint8_t* hit,
                                         unsigned long long*, hipStream_t s) {
    const BoxRefineCtx& cx = *(const BoxRefineCtx*)ctx;
    GPK_LAUNCH("gpk_pair_contains", pair_contains_kernel, pair_group_grid(n_cand), dim3(256), 0, s, cx.left->d, cx.right->d, cand_l, cand_r,
               (int64_t)n_cand, cx.lbbox, cx.rbbox, hit);
    return GPK_OK;
}
static int32_t refine_lineal_point(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void*, uint8_t* hit,
                                   unsigned long long*, hipStream_t s) {
    const BoxRefineCtx& cx = *(const BoxRefineCtx*)ctx;
    GPK_LAUNCH("gpk_lineal_point_refine", lineal_point_refine_kernel, dim3((unsigned)(((int64_t)n_cand + 255) / 256)), dim3(256), 0, s, cx.left->d,
               cx.right->d, cand_l, cand_r, (int64_t)n_cand, hit);
    return GPK_OK;
}
template <int CONTAINED>
static int32_t refine_envelope(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void*, uint8_t* hit, unsigned long long*,
                               hipStream_t s) {
    const BoxRefineCtx& cx = *(const BoxRefineCtx*)ctx;
    GPK_LAUNCH("gpk_envelope_refine", envelope_refine_kernel, dim3((unsigned)(((int64_t)n_cand + 255) / 256)), dim3(256), 0, s, cand_l, cand_r,
               (int64_t)n_cand, cx.lbbox, cx.rbbox, CONTAINED, hit);
    return GPK_OK;
}
// (no scratch, nothing to gather; their errors carry gpk_spatial_join's name, as gpk_index_query_envelope's always did)
static CandRefine builtin_refine(BoxRefineCtx* cx, decltype(CandRefine::refine) refine) { return CandRefine{"spatial_join", cx, 0, 0, refine, nullptr}; }
CandRefine polygonal_intersects_refine(BoxRefineCtx* cx) { return builtin_refine(cx, refine_polygonal_intersects); }
CandRefine polygonal_contains_refine(BoxRefineCtx* cx) { return builtin_refine(cx, refine_polygonal_contains); }
CandRefine lineal_point_refine(BoxRefineCtx* cx) { return builtin_refine(cx, refine_lineal_point); }
BoxRefineCtx box_refine_ctx(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, const double4* lbbox) {
    return BoxRefineCtx{left, right, lbbox, right_index->v.bbox, left->d.type == GPK_GEOM_POLYGON && left->classes && left->classes->one_to_one,
                        right->d.type == GPK_GEOM_POLYGON && right->classes && right->classes->one_to_one};
}

int32_t left_boxes(const gpk_geoarray* left, hipStream_t s, const double4** out) {
    const int64_t n = left->d.n_geoms;
    Scratch sc(workspace_aux(0));
    double4* lbbox;
    sc.add(lbbox, (size_t)n);
    GPK_TRY(sc.commit());
    *out = lbbox;
    return gpk_bounds(left, (double*)lbbox, GPK_MEM_DEVICE, (void*)s);
}

// candidates (count, scan, fill) -> the caller's refine -> hits (count, scan, emit)
int32_t bbox_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, uint32_t left_row_base,
                  uint32_t* out_counts, uint32_t* out_pairs, int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, hipStream_t s,
                  const double4* lbbox, const CandRefine& refine) {
    const int64_t n = left->d.n_geoms;
    const char* what = refine.name;
    const bool want_pairs = pair_capacity > 0;
    // left boxes and the candidate buffers live in the thread's auxiliary arenas (no hipMalloc / hipFree per call)
    // (a caller's lbbox — in device memory — takes the left boxes' place: query boxes, boxes grown by a distance)
    if (!lbbox) GPK_TRY(left_boxes(left, s, &lbbox));
    const int64_t nb = (n + 255) / 256;
    // (padded staging of the candidates: up to 512 MB — 8M left rows; beyond that the two-search path)
    const size_t stage_words = CAND_STAGE * (size_t)(n > 0 ? n : 1);
    const bool staged = sizeof(uint32_t) * stage_words <= (size_t(512) << 20);
    Scratch sc(workspace());
    int32_t *cand_cnt, *cand_off, *counts, *offsets, *big_rows;
    unsigned long long* btot;
    uint32_t *counts_out, *pairs_dev, *stage;
    sc.add_n((size_t)(n + 1), cand_cnt, cand_off, counts, offsets);
    sc.add(btot, (size_t)(nb + 2));
    sc.add(big_rows, 64);
    sc.stage(counts_out, out_counts, out_space, (size_t)n);
    sc.stage(pairs_dev, want_pairs ? out_pairs : nullptr, out_space, 2 * (size_t)pair_capacity);
    sc.add_if(staged, stage, stage_words);
    GPK_TRY(sc.commit());

    // stage 1: candidates per left row
    GPK_HIP(hipMemsetAsync(big_rows, 0, 2 * sizeof(int32_t), s));
    if (staged)
        GPK_LAUNCH("gpk_bbox_cand_count", bbox_cand_stage_kernel, dim3((unsigned)((n * CAND_LANES + 255) / 256)), dim3(256), 0, s, left->d, right->d,
                   right_index->v, lbbox, cand_cnt, stage, big_rows);
    else
        GPK_LAUNCH("gpk_bbox_cand_count", bbox_cand_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, left->d, right->d, right_index->v,
                   lbbox, cand_cnt, (const int32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, big_rows);
    GPK_TRY(exclusive_scan_i32(cand_cnt, n, cand_off, nullptr, btot, s));
    unsigned long long cand_total = 0;  // the 64-bit grand total of the scan: cand_off[n] is its truncation to i32
    int32_t fl[2] = {0, 0};
    GPK_HIP(hipMemcpyAsync(&cand_total, btot + nb, sizeof cand_total, hipMemcpyDeviceToHost, s));
    GPK_HIP(hipMemcpyAsync(fl, big_rows, sizeof fl, hipMemcpyDeviceToHost, s));
    GPK_HIP(hipStreamSynchronize(s));
    const int32_t has_big_rows = fl[0];
    // candidate offsets are i32 (one slice per left row): more than 2^31 - 1 bbox candidates cannot be addressed
    if (cand_total > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_CAPACITY, "%s: %llu bbox candidates exceed the i32 candidate offsets: shard the left side", what, cand_total);
    const int32_t n_cand = (int32_t)cand_total;
    uint32_t* cand_sorted = nullptr;
    void *seg_tmp = nullptr, *scratch = nullptr;
    size_t seg_bytes = 0;
    unsigned seg_bits = 1;
    while (seg_bits < 32 && ((int64_t)1 << seg_bits) < right->d.n_geoms) ++seg_bits;
    const size_t nc1 = (size_t)(n_cand > 0 ? n_cand : 1);
    if (has_big_rows) {
        const hipError_t qe = rocprim::segmented_radix_sort_keys(nullptr, seg_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (unsigned)n_cand,
                                                                 (unsigned)n, (const int32_t*)cand_off, (const int32_t*)cand_off + 1, 0, seg_bits, s);
        if (qe != hipSuccess) return fail(GPK_ERR_DEVICE, "%s: %s", what, hipGetErrorString(qe));
    }
    const size_t scratch_bytes = align256(refine.scratch_fixed + refine.scratch_per_cand * nc1);
    Scratch sc1(workspace_aux(1));
    uint32_t *cand_r, *cand_l;
    uint8_t* hit;
    sc1.add_n(nc1, cand_r, cand_l, hit);
    if (has_big_rows) {
        sc1.add(cand_sorted, nc1);
        sc1.add_bytes(seg_tmp, seg_bytes);
    }
    if (scratch_bytes) sc1.add_bytes(scratch, scratch_bytes);
    GPK_TRY(sc1.commit());

    // stages 2 and 3: the candidate lists, the refine, the hits
    if (staged && !has_big_rows)
        GPK_LAUNCH("gpk_cand_compact", cand_compact_kernel, dim3((unsigned)((n * CAND_STAGE + 255) / 256)), dim3(256), 0, s, left->d, right->d,
                   right_index->v, (const double4*)lbbox, (const int32_t*)cand_cnt, (const int32_t*)cand_off, (const uint32_t*)stage, cand_r, cand_l);
    else
        GPK_LAUNCH("gpk_bbox_cand_fill", bbox_cand_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, left->d, right->d, right_index->v,
                   lbbox, cand_cnt, (const int32_t*)cand_off, cand_r, cand_l, big_rows);
    if (has_big_rows && n_cand > 0) {  // some slice is long: sort every slice by right id, segment = left row
        GPK_HIP(rocprim::segmented_radix_sort_keys(seg_tmp, seg_bytes, (const uint32_t*)cand_r, cand_sorted, (unsigned)n_cand, (unsigned)n,
                                                   (const int32_t*)cand_off, (const int32_t*)cand_off + 1, 0, seg_bits, s));
        cand_r = cand_sorted;
    }
    if (n_cand > 0) GPK_TRY(refine.refine(refine.ctx, cand_l, cand_r, n_cand, scratch, hit, join_stats_buffer(), s));
    GPK_LAUNCH("gpk_pair_count", pair_emit_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, n, (const int32_t*)cand_off,
               (const uint32_t*)cand_r, (const uint8_t*)hit, counts, (const int32_t*)nullptr, left_row_base, (uint2*)nullptr, (int64_t)0);
    GPK_TRY(exclusive_scan_i32(counts, n, offsets, nullptr, btot, s));
    if (counts_out)
        GPK_LAUNCH("gpk_counts_copy", i32_to_u32_copy_kernel, dim3((unsigned)nb), dim3(256), 0, s, counts, counts_out, n);
    if (want_pairs)
        GPK_LAUNCH("gpk_pair_emit", pair_emit_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, n, (const int32_t*)cand_off,
                   (const uint32_t*)cand_r, (const uint8_t*)hit, counts, (const int32_t*)offsets, left_row_base, (uint2*)pairs_dev,
                   pair_capacity);
    if (want_pairs && refine.emitted) GPK_TRY(refine.emitted(refine.ctx, n, cand_off, hit, offsets, scratch, pair_capacity, s));
    if (want_pairs && refine.emitted_pairs) GPK_TRY(refine.emitted_pairs(refine.ctx, offsets, left_row_base, pairs_dev, pair_capacity, s));
    unsigned long long total = 0;  // 64-bit grand total of the hit scan (hits <= candidates <= INT32_MAX, checked above)
    hipError_t e = hipMemcpyAsync(&total, btot + nb, sizeof total, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(GPK_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
    return finish_pairs(what, (int64_t)total, n, out_counts, counts_out, out_pairs, pairs_dev, pair_capacity, n_pairs, out_space, s);
}

// ---- bbox_join with a value per pair (gpk_candjoin.h) ----------------------------------------------------------------------------
static int32_t payload_emitted(void* ctx, int64_t n_rows, const int32_t* cand_off, const uint8_t* hit, const int32_t* offsets, void* scratch,
                               int64_t pair_capacity, hipStream_t s) {
    const PayloadCtx& cx = *(const PayloadCtx*)ctx;
    if (!cx.payload_out) return GPK_OK;
    const dim3 grid((unsigned)((n_rows + 255) / 256));
    const void* payload = (const char*)scratch + 256;
    if (cx.payload_elem == sizeof(uint8_t))
        GPK_LAUNCH(cx.gather_label, (payload_gather_kernel<uint8_t>), grid, dim3(256), 0, s, n_rows, cand_off, hit, offsets, (const uint8_t*)payload,
                   (uint8_t*)cx.payload_out, pair_capacity);
    else
        GPK_LAUNCH(cx.gather_label, (payload_gather_kernel<double>), grid, dim3(256), 0, s, n_rows, cand_off, hit, offsets, (const double*)payload,
                   (double*)cx.payload_out, pair_capacity);
    return GPK_OK;
}

int32_t payload_join(const PayloadJoin& join, const gpk_index* right_index, uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs,
                     void* out_payload, int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream) {
    PayloadCtx& cx = *join.ctx;
    const gpk_geoarray *left = cx.left, *right = cx.right;
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = left->d.n_geoms;
    if (n == 0) return GPK_OK;
    if (n > (int64_t)INT32_MAX) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: more than 2^31 - 1 left rows: shard the left side", join.who);
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
    const bool want_payload = out_payload && pair_capacity > 0;
    Scratch sc(workspace_aux(0));
    double4 *lbox, *other;
    uint8_t* payload_dev;
    sc.add(lbox, (size_t)n);
    sc.add_if(join.boxes != nullptr, other, (size_t)n);
    sc.stage(payload_dev, want_payload ? (uint8_t*)out_payload : nullptr, out_space, cx.payload_elem * (size_t)pair_capacity);
    int32_t rc = sc.commit();
    if (rc != GPK_OK) return finish(rc);
    cx.payload_out = payload_dev;
    rc = gpk_bounds(left, (double*)lbox, GPK_MEM_DEVICE, stream);
    if (rc == GPK_OK && join.boxes) rc = join.boxes(&cx, right_index, lbox, other, n, s);
    if (rc != GPK_OK) return finish(rc);

    CandRefine hook;
    hook.name = join.who;
    hook.ctx = &cx;
    hook.scratch_fixed = 512;
    hook.scratch_per_cand = (cx.payload_out ? cx.payload_elem : 0) + join.extra_per_cand;
    hook.refine = join.refine;
    hook.emitted = join.emitted_pairs ? nullptr : payload_emitted;
    hook.emitted_pairs = join.emitted_pairs;
    rc = bbox_join(left, right, right_index, left_row_base, out_counts, out_pairs, pair_capacity, n_pairs, out_space, s, other ? other : lbox, hook);
    if (rc != GPK_OK) return finish(rc);
    if (want_payload && host_out && *n_pairs > 0) {
        const int64_t got = *n_pairs < pair_capacity ? *n_pairs : pair_capacity;
        rc = copy_out(out_payload, out_space, cx.payload_out, cx.payload_elem * (size_t)got, s);
    }
    return finish(rc);
}

}  // namespace gpk

using namespace gpk;

extern "C" {

int32_t gpk_index_query_envelope(const gpk_index* idx, const double* boxes4, int64_t n_boxes, int32_t mode, uint32_t* out_counts,
                                 uint32_t* out_pairs, int64_t pair_capacity, int64_t* n_pairs, int32_t space, void* stream) {
    if (!idx || !n_pairs || (n_boxes > 0 && !boxes4)) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (mode != GPK_QUERY_CONTAINED && mode != GPK_QUERY_INTERSECTING) return fail(GPK_ERR_INVALID_ARGUMENT, "unknown envelope query mode %d", mode);
    if (n_boxes < 0 || pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "bad sizes");
    if (n_boxes > (int64_t)0x7FFFFFF0ll) return fail(GPK_ERR_INVALID_ARGUMENT, "more than 2^31 query boxes");
    *n_pairs = 0;
    GPK_TRY(require_device());
    if (n_boxes == 0) return GPK_OK;
    hipStream_t s = (hipStream_t)stream;
    // the queries take the left rows' place in the box join, the index's own array the right rows' (the index holds the leaves: no
    // geometry is read); null and empty rows of the indexed array have NaN boxes and are in no directory cell
    gpk_geoarray left, right;
    memset(&left, 0, sizeof left);
    memset(&right, 0, sizeof right);
    left.d.type = GPK_GEOM_POINT;
    left.d.n_geoms = n_boxes;
    left.device = right.device = idx->device;
    right.d.type = idx->geom_type;
    right.d.n_geoms = idx->n_geoms;
    // the queries in the library's own memory, corners ordered the way `AABB::from_corners` orders them (lower = the component-wise
    // minimum of the two corners, upper = the maximum)
    Scratch sc(workspace_aux(0));
    double4* boxes_dev;
    const double4* src;
    sc.add(boxes_dev, (size_t)n_boxes);
    sc.stage_in(src, reinterpret_cast<const double4*>(boxes4), space, (size_t)n_boxes);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    GPK_LAUNCH("gpk_query_boxes", query_boxes_kernel, dim3((unsigned)((n_boxes + 255) / 256)), dim3(256), 0, s, src, n_boxes, boxes_dev);
    BoxRefineCtx cx = box_refine_ctx(&left, &right, idx, boxes_dev);
    return bbox_join(&left, &right, idx, 0u, out_counts, out_pairs, pair_capacity, n_pairs, space, s, boxes_dev,
                     builtin_refine(&cx, mode == GPK_QUERY_CONTAINED ? refine_envelope<1> : refine_envelope<0>));
}

}  // extern "C"
