// gpk_pointrel.hip — point relations: the row-wise mask (gpk_point_relation) and the predicate join (gpk_point_relation_join) over the
// routine of gpk_pointrel.h.  Contract: include/geopolars_hip.h.
//
// A unit is a pair (row of A, row of B): row i against row rows[i] for the row-wise call, a candidate (l, r) for the join, where A is
// the punctual side.  One kernel serves both, with two schedules:
//   point_relation_kernel<G, ONE>   G lanes per unit, G = 4 or 16 (ll::relation_group_size's rule over B's column, and over A's when it
//                                   is a MULTIPOINT column).  ONE: A is a POINT column — one point, no outer loop, no set comparison.
//                                   Exactly one lane group per unit: ceil(n / (256 / G)) blocks, no cap, no unit loop, nothing carried
//                                   from one unit to the next.  A unit of a MULTIPOINT column with n_A * n_B > PT_LARGE_COST that
//                                   pt::prepare did not settle is appended to a list, what is known of its mask left in its state byte.
//   point_relation_large_kernel     one 256-lane work-group per listed unit.  Thread t owns the points t, t + 256, ... of A; B is staged
//                                   in LDS, PT_CHUNK elements (coordinate, end of its segment, member ends) at a time, and every
//                                   thread walks the chunk with uniform LDS reads.  B comes from global memory once per round of 256
//                                   points (once altogether when it fits one chunk), not once per point.  Bit 8 of a finite B is the same
//                                   walk with the sides exchanged.  A fixed grid of PT_LIST_BLOCKS work-groups loops over the list and
//                                   reads its length on the device: no read-back.
// A POINT column never lists a unit: its one point strides B over the G lanes whatever B's size (correct and slow for a B of many
// thousand coordinates, as the sibling relations are).
//
// Join: payload_join (gpk_candjoin.h) with the left rows' own boxes.  The refine runs the kernel on the candidates with A = the punctual
// side (the left one when both are) and the predicate transposed when that is the right side; hit = predicate(mask, dim B).  When the
// caller asks for the per-pair masks the full mask is computed and gathered after the emit; otherwise the work on a pair ends as soon as
// its predicate is settled (pt::stop_of).  `left` and `right` may be one array.
#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_linearea.h"
#include "gpk_pairdist.h"
#include "gpk_pointrel.h"

namespace gpk {

namespace {

constexpr int PT_CHUNK = 1024;             // elements of the walked side staged in LDS per round (33 KB)
constexpr unsigned PT_LIST_BLOCKS = 1024;  // four work-groups a compute unit on the 256-CU part this library targets

struct DevOrient {
    __device__ int operator()(pt::P2 a, pt::P2 b, pt::P2 c) const { return dev::orient2d(a.x, a.y, b.x, b.y, c.x, c.y); }
};

__host__ __device__ inline bool is_punctual(int32_t t) { return t == GPK_GEOM_POINT || t == GPK_GEOM_MULTIPOINT; }
__host__ __device__ inline int family_dim(int32_t t) { return is_punctual(t) ? 0 : (is_lineal(t) ? 1 : 2); }
inline bool known_family(int32_t t) { return is_punctual(t) || is_lineal(t) || is_polygonal(t); }

// row j of any family as the routine's view; false: null or out of range
__device__ __forceinline__ bool pt_row(const DevGeo& g, int64_t j, pt::Row& r) {
    if (!dev::row_ok(g, j)) return false;
    r = pt::Row{reinterpret_cast<const pt::P2*>(g.xy), nullptr, 0, 0, 0, 0, family_dim(g.type)};
    if (g.type == GPK_GEOM_POINT) {
        r.c0 = (int)j;
        r.c1 = (int)j + 1;
        return true;
    }
    int s0 = g.geom_off[j], s1 = g.geom_off[j + 1];
    if (g.type == GPK_GEOM_MULTIPOINT) {
        r.c0 = s0;
        r.c1 = s1;
        return true;
    }
    if (g.type == GPK_GEOM_LINESTRING) {
        r.so = g.geom_off;
        s0 = (int)j;
        s1 = (int)j + 1;
    } else {
        r.so = g.ring_off;
        if (g.type == GPK_GEOM_MULTIPOLYGON) {
            s0 = g.part_off[s0];
            s1 = g.part_off[s1];
        }
    }
    r.s0 = s0;
    r.s1 = s1;
    r.c0 = r.so[s0];
    r.c1 = r.so[s1];
    return true;
}

// The units of a launch: unit u is row ia[u] of A (u itself without a list) against row ib[u] of B.  `hit` (the join): predicate(mask);
// `mask` (the row-wise call, and the join when the masks were asked for): the mask.  The state byte of a listed unit is hit[u] for the
// join and mask[u] for the row-wise call.
struct Units {
    const uint32_t *ia, *ib;
    int64_t n;
    int predicate;  // (unused without `hit`)
    pt::Stop st;
    uint8_t *hit, *mask;
};
__device__ __forceinline__ void store_unit(const Units& u, int64_t k, int mask, int dim_b) {
    if (u.hit) u.hit[k] = pt::predicate_of(mask, u.predicate, dim_b) ? 1 : 0;
    if (u.mask) u.mask[k] = (uint8_t)mask;
}

template <int G, bool ONE>
__global__ __launch_bounds__(256) void point_relation_kernel(DevGeo a, DevGeo b, Units u, uint32_t* __restrict__ large, uint32_t* __restrict__ n_large) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t k = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;  // one lane group per unit: the whole group leaves together
    if (k >= u.n) return;
    const int64_t i = u.ia ? (int64_t)u.ia[k] : k, j = u.ib ? (int64_t)u.ib[k] : k;
    const int dim_b = family_dim(b.type);
    pt::Row A, B;
    int mask = 0;
    if (pt_row(a, i, A) && pt_row(b, j, B)) {
        const pt::Pre pre = pt::prepare<G>(A, B, lane, u.st, DevOrient{});
        mask = pre.mask;
        if (!pre.settled) {
            if (!ONE && (int64_t)(A.c1 - A.c0) * (B.c1 - B.c0) > pt::PT_LARGE_COST) {
                if (lane == 0) {
                    (u.hit ? u.hit : u.mask)[k] = (uint8_t)(mask | (pre.b_finite ? pt::PENDING : 0));
                    large[atomicAdd(n_large, 1u)] = (uint32_t)k;
                }
                return;
            }
            mask = pt::finish<G, ONE>(A, B, pre, lane, u.st, DevOrient{});
        }
    }
    if (lane == 0) store_unit(u, k, mask, dim_b);
}

struct PtLds {
    double4 seg[PT_CHUNK];
    uint8_t ends[PT_CHUNK];
    int bits;
};

// The bits 1, 2, 4 of the points of W against the row O by the whole work-group; ends once done(seen | bits, st).  Same value on every
// thread.  Ends with a barrier: the LDS can be reused at once.
__device__ int classify_workgroup(const pt::Row& W, const pt::Row& O, PtLds& lds, int seen, pt::Stop st) {
    const int tid = threadIdx.x;
    const int nw = W.c1 - W.c0, no = O.c1 - O.c0;
    const bool one_chunk = no <= PT_CHUNK;
    if (tid == 0) lds.bits = 0;
    int mask = 0;
    for (int u0 = 0; u0 < nw; u0 += 256) {
        const bool active = u0 + tid < nw;
        const pt::P2 p = active ? W.xy[W.c0 + u0 + tid] : pt::P2{0.0, 0.0};
        pt::Acc acc{0, 0, 0};
        for (int ch = 0; ch < no; ch += PT_CHUNK) {
            const int len = no - ch < PT_CHUNK ? no - ch : PT_CHUNK;
            if (!one_chunk || u0 == 0) {
                __syncthreads();  // the previous chunk is no longer read
                for (int t = tid; t < len; t += 256) {
                    const int c = O.c0 + ch + t;
                    const pt::P2 v = O.xy[c];
                    pt::P2 w = v;
                    int ends = 0;
                    if (O.so) {
                        const int s = seq_of(O.so, O.s0, O.s1, c);
                        if (c + 1 < O.so[s + 1]) w = O.xy[c + 1];
                        ends = (c == O.so[s] ? 1 : 0) + (c + 1 == O.so[s + 1] ? 1 : 0);
                    }
                    lds.seg[t] = make_double4(v.x, v.y, w.x, w.y);
                    lds.ends[t] = (uint8_t)ends;
                }
                __syncthreads();
            }
            if (active) {
                for (int t = 0; t < len; ++t) {
                    const double4 s = lds.seg[t];
                    pt::see(acc, p, pt::P2{s.x, s.y}, pt::P2{s.z, s.w}, (int)lds.ends[t], O.dim, DevOrient{});
                }
            }
        }
        if (active) atomicOr(&lds.bits, pt::bit_of(acc.on, acc.cross, acc.ends, O.dim));
        __syncthreads();
        mask = lds.bits;
        __syncthreads();  // every thread has read the word before the next round adds to it
        if (pt::done(seen | mask, st)) break;
    }
    __syncthreads();
    return mask;
}

__global__ __launch_bounds__(256) void point_relation_large_kernel(DevGeo a, DevGeo b, Units u, const uint32_t* __restrict__ large,
                                                                   const uint32_t* __restrict__ n_large) {
    __shared__ PtLds lds;
    const uint32_t count = *n_large;
    const int dim_b = family_dim(b.type);
    uint8_t* state = u.hit ? u.hit : u.mask;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const int64_t k = large[e];
        const int64_t i = u.ia ? (int64_t)u.ia[k] : k, j = u.ib ? (int64_t)u.ib[k] : k;
        pt::Row A, B;
        (void)pt_row(a, i, A);  // (a listed unit has two usable rows)
        (void)pt_row(b, j, B);
        const int st0 = state[k];
        int mask = st0 & pt::PT_ALL;
        mask |= classify_workgroup(A, B, lds, mask, u.st);
        if ((st0 & pt::PENDING) && !pt::done(mask, u.st)) {
            // B is a finite set: each of its points against the set A
            pt::Row as_set = A;
            as_set.dim = 0;
            as_set.so = nullptr;
            if (classify_workgroup(B, as_set, lds, 0, pt::Stop{pt::EXTERIOR, pt::PT_ALL}) & pt::EXTERIOR) mask |= pt::B_OUTSIDE;
        }
        if (threadIdx.x == 0) store_unit(u, k, mask, dim_b);
    }
}

// lanes per unit, ll::relation_group_size's rule: B's mean coordinate count decides, and A's when its points are a list
int group_size(const DevGeo& a, const DevGeo& b) {
    const int gb = b.type == GPK_GEOM_POINT ? lp::LP_G_SMALL : lp::relation_group_size(b, b);
    const int ga = a.type == GPK_GEOM_POINT ? lp::LP_G_SMALL : lp::relation_group_size(a, a);
    return ga > gb ? ga : gb;
}

// both launches of a call over the units `u` (A = a, B = b); `large` holds u.n entries, `n_large` one word (zeroed here)
int32_t launch_units(const char* label, const char* label_large, const DevGeo& a, const DevGeo& b, const Units& u, uint32_t* large, uint32_t* n_large,
                     hipStream_t s) {
    const bool one = a.type == GPK_GEOM_POINT;
    const int G = group_size(a, b);
    // exactly one lane group per unit: ceil(n / (256 / G)) blocks, no cap and no unit loop in the kernel
    const int64_t per_block = 256 / G;
    const dim3 grid((unsigned)((u.n + per_block - 1) / per_block)), block(256);
    if (!one) GPK_HIP(hipMemsetAsync(n_large, 0, sizeof(uint32_t), s));
    if (one && G == lp::LP_G_SMALL)
        GPK_LAUNCH(label, (point_relation_kernel<lp::LP_G_SMALL, true>), grid, block, 0, s, a, b, u, large, n_large);
    else if (one)
        GPK_LAUNCH(label, (point_relation_kernel<lp::LP_G_LARGE, true>), grid, block, 0, s, a, b, u, large, n_large);
    else if (G == lp::LP_G_SMALL)
        GPK_LAUNCH(label, (point_relation_kernel<lp::LP_G_SMALL, false>), grid, block, 0, s, a, b, u, large, n_large);
    else
        GPK_LAUNCH(label, (point_relation_kernel<lp::LP_G_LARGE, false>), grid, block, 0, s, a, b, u, large, n_large);
    // the listed units: a fixed grid of work-groups (the device's CU count is not asked) that loops over the list and reads its length
    // on the device
    if (!one)
        GPK_LAUNCH(label_large, point_relation_large_kernel, dim3(PT_LIST_BLOCKS), block, 0, s, a, b, u, (const uint32_t*)large, (const uint32_t*)n_large);
    return GPK_OK;
}

struct PtCtx {
    PayloadCtx p;  // (p.payload_out: the masks were asked for)
    int32_t predicate;  // as a predicate of (A, B)
    bool a_is_right;
};

// scratch of a call: 256 bytes of counters (word 0: listed candidates), then mask[n_cand] when the masks were asked for, then the list
// [n_cand] on the next 4-byte boundary
int32_t pt_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit, unsigned long long* stats,
                  hipStream_t s) {
    (void)stats;
    const PtCtx& cx = *(const PtCtx*)ctx;
    const DevGeo& A = cx.a_is_right ? cx.p.right->d : cx.p.left->d;
    const DevGeo& B = cx.a_is_right ? cx.p.left->d : cx.p.right->d;
    char* p = (char*)scratch;
    uint32_t* n_large = (uint32_t*)p;
    p += 256;
    uint8_t* mask = cx.p.payload_out ? (uint8_t*)p : nullptr;
    if (mask) p += ((size_t)n_cand + 3) & ~(size_t)3;
    uint32_t* large = (uint32_t*)p;
    const pt::Stop st = mask ? pt::Stop{0, pt::PT_ALL} : pt::stop_of(cx.predicate);
    const Units u{cx.a_is_right ? cand_r : cand_l, cx.a_is_right ? cand_l : cand_r, (int64_t)n_cand, (int)cx.predicate, st, hit, mask};
    return launch_units("gpk_point_relation_refine", "gpk_point_relation_refine_large", A, B, u, large, n_large, s);
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_point_relation(const gpk_geoarray* points, const gpk_geoarray* other, const uint32_t* other_rows, uint8_t* out_mask,
                                      int32_t out_space, void* stream) {
    if (!points || !other || !out_mask) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_punctual(points->d.type) || !known_family(other->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "point_relation: POINT | MULTIPOINT x any of the six families (found types %d, %d)", points->d.type,
                    other->d.type);
    auto launch = [&](const uint32_t* rows_dev, void* out_dev, int64_t n, hipStream_t s) -> int32_t {
        Scratch sc(workspace_aux(0));
        uint32_t *large, *n_large;
        const bool lists = points->d.type != GPK_GEOM_POINT;  // (a POINT column lists nothing)
        sc.add_if(lists, large, (size_t)n);
        sc.add_if(lists, n_large, 1);
        GPK_TRY(sc.commit());
        const Units u{nullptr, rows_dev, n, 0, pt::Stop{0, pt::PT_ALL}, nullptr, (uint8_t*)out_dev};
        return launch_units("gpk_point_relation", "gpk_point_relation_large", points->d, other->d, u, large, n_large, s);
    };
    return rowwise_pairs("point_relation", points, other, other_rows, out_mask, 1, out_space, stream, launch);
}

extern "C" int32_t gpk_point_relation_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t predicate,
                                           uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, uint8_t* out_mask,
                                           int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (predicate < GPK_PT_PRED_INTERSECTS || predicate > GPK_PT_PRED_EQUALS)
        return fail(GPK_ERR_INVALID_ARGUMENT, "point_relation_join: unknown predicate %d", predicate);
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    const int32_t tl = left->d.type, tr = right->d.type;
    if (!known_family(tl) || !known_family(tr) || (!is_punctual(tl) && !is_punctual(tr))) {
        const char* own = !known_family(tl) || !known_family(tr)       ? "no relation join takes these types"
                          : is_lineal(tl) && is_lineal(tr)             ? "two line columns: gpk_line_relation_join"
                          : is_polygonal(tl) && is_polygonal(tr)       ? "two polygon columns: gpk_polygon_relation_join"
                                                                       : "lines and polygons: gpk_line_polygon_join";
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "point_relation_join: one side must be POINT | MULTIPOINT (found types %d, %d; %s)", tl, tr, own);
    }
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "point_relation_join"));
    const bool a_is_right = !is_punctual(tl);
    const int32_t pred = a_is_right ? pt::transposed(predicate) : predicate;
    if (!pt::can_hold(pred, family_dim(a_is_right ? tl : tr))) {  // never true for this pair of families: every count is zero
        GPK_TRY(require_device());
        GPK_TRY(zero_counts(out_counts, left->d.n_geoms, out_space, (hipStream_t)stream));
        if (out_counts && out_space == GPK_MEM_DEVICE) GPK_HIP(hipStreamSynchronize((hipStream_t)stream));
        return GPK_OK;
    }
    PtCtx cx{{left, right, "gpk_point_relation_gather", sizeof(uint8_t), nullptr}, pred, a_is_right};
    return payload_join(PayloadJoin{"point_relation_join", &cx.p, pt_refine, sizeof(uint32_t), nullptr}, right_index, left_row_base, out_counts, out_pairs,
                        out_mask, pair_capacity, n_pairs, out_space, stream);
}
