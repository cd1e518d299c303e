// gpk_knn.hip — k-nearest-neighbours join for any two of POINT, MULTIPOINT, LINESTRING, MULTILINESTRING, POLYGON and MULTIPOLYGON: for every
// left row the k right rows with the smallest keys (bits(d), r), nearest first.  Contract: include/geopolars_hip.h (gpk_knn_join).
//
// Pipeline (payload_join of gpk_candjoin.h: its `boxes` hook does steps 1-2, its refine steps 3-4, its `emitted_pairs` hook step 5):
//   1. k-seed walk (knn_walk_kernel, the rule of gpk_knnwalk.h, one lane per left row, the row's K slots in LDS): the K = k (k + 1 with
//      GPK_KNN_EXCLUDE_SELF: one of them may be the row itself) distinct usable right rows whose boxes have the smallest FAR distance
//      to the left row's box, among those with far distance <= max_distance.  No coordinate is read.
//   2. radius r_l, in the same kernel: K rows found: min(max_distance, F_K + m), F_K the K-th far distance; fewer: max_distance (with
//      INFINITY the right side then has fewer than K usable rows at all); a null left row or one without a usable box: NaN.  The left box
//      grown on every side by r_l + margin takes the left box's place in the candidate search; a NaN radius gives a NaN box, which lists
//      no candidates.
//   3. candidates (the staged bbox candidate generator) and their exact distances: refine_row_candidates of gpk_dwithin.hip with r_l as
//      the threshold of the box pre-test — the routines, group sizes and lane orders of gpk_distance_rowwise's per-row kernels, the
//      work-group routine above PD_LARGE_COST: d is bit for bit the double that call returns.
//   4. selection: a candidate is eligible when d <= r_l and it is not the self pair; its rank is the number of the row's eligible keys
//      below its own, and hit = rank < k.  Keys of a row are distinct (the right rows are), so the hits' ranks are 0 .. count - 1.
//        knn_select_wave_kernel   one wave per left row, one key per lane, rank by cross-lane comparison: rows of up to 64 candidates.
//                                 Longer rows are appended to a list.
//        knn_select_list_kernel   a fixed grid of KNN_LIST_BLOCKS work-groups loops over that list, a row per work-group at a time.
//                                 Up to KNN_LDS_KEYS candidates: the keys in LDS (12 bytes each), rank by comparison with every other.
//                                 More: radix select of the k-th key over the 96-bit key, twelve 8-bit passes over the row in global
//                                 memory with a histogram in LDS, then the at most 64 keys up to it are ranked in LDS.
//      The two thresholds (64: the wave; KNN_LDS_KEYS) are not tuned by measurement.
//   5. the generator's count / scan gives counts and offsets; knn_emit_kernel writes the hit with rank j to pair slot offsets[l] + j and
//      its distance beside it, from the candidate arrays: pairs sorted by (l, d, r).
//
// Why no neighbour is lost.  The far distance of two boxes bounds the exact distance D of the rows from above, and the computed d
// exceeds D by at most 16 u (D + 2 lmax), which m = 64 eps (|x0| + |y0| + extent width + extent height + the left box's |coordinates|
// + F_K) covers several times over.  So when K rows were found, K distinct usable rows — k of them not the row itself — have
// d <= r_l or d > max_distance; otherwise r_l = max_distance.  Either way the k-th eligible key's distance is at most r_l, and every
// row up to it has d <= r_l.  From here the margin argument at the top of gpk_dwithin.hip carries over with r_l in `distance`'s place,
// as in gpk_nearest_any.hip: the boxes are exact, the gap between them along either axis is at most D, so the right box's edge lies
// within the left box grown by g = fl(r_l + m'), m' of the same form around r_l.  The candidate generator compares the grown box with
// the right boxes and assigns cells with the directory's own monotone cell function, exactly; the refine's box pre-test uses the same
// form of margin, and a candidate it rejects has a distance above r_l.
//
// The result does not depend on scheduling: the walk is sequential per row, the distances are those of fixed lane orders, a rank is a
// count of smaller keys, and the order in which long rows enter the list only decides which work-group ranks them.
//
// Never matched: null rows, rows without a coordinate and POINT rows with a NaN coordinate have a NaN box (or are refused by the
// candidate kernels' validity test): no radius on the left, never a seed or a candidate on the right.
#include <cfloat>
#include <cmath>

#include "gpk_candjoin.h"
#include "gpk_device.h"
#include "gpk_dwithin_refine.h"
#include "gpk_knnwalk.h"

namespace gpk {

namespace {

constexpr int KNN_WALK_LANES = 64;          // left rows per work-group of the walk: K * 64 slots of 12 bytes in LDS (at most 49 920 bytes)
constexpr unsigned KNN_LIST_BLOCKS = 1024;  // four work-groups a compute unit on the 256-CU part this library targets
constexpr int KNN_LDS_KEYS = 2048;          // longest row ranked from LDS (24 KB of keys)
constexpr uint8_t NO_RANK = 0xFF;
constexpr unsigned long long BAD_KEY = ~0ull;  // above the bits of every distance, INFINITY included

struct KnnDir {
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

// a lane's K slots: slot s of lane t at [s * KNN_WALK_LANES + t], so that the lanes of a wave touch consecutive words
struct LdsSlots {
    double* f;
    uint32_t* r;
    __device__ __forceinline__ double& far(int s) { return f[s * KNN_WALK_LANES]; }
    __device__ __forceinline__ uint32_t& row(int s) { return r[s * KNN_WALK_LANES]; }
};

// Steps 1-2.  Dynamic LDS: K * KNN_WALK_LANES doubles, then as many words.
__global__ __launch_bounds__(KNN_WALK_LANES) void knn_walk_kernel(nw::Grid g, KnnDir dir, const double4* __restrict__ lbox,
                                                                  const uint8_t* __restrict__ lvalid, int64_t n, double max_d, int K,
                                                                  double* __restrict__ radius, double4* __restrict__ grown) {
    extern __shared__ double knn_walk_lds[];
    const int64_t i = (int64_t)blockIdx.x * KNN_WALK_LANES + threadIdx.x;
    if (i >= n) return;
    LdsSlots slots{knn_walk_lds + threadIdx.x, (uint32_t*)(knn_walk_lds + (size_t)K * KNN_WALK_LANES) + threadIdx.x};
    const double4 b = lbox[i];
    const nw::Box L{b.x, b.y, b.z, b.w};
    double r = NAN;
    if (dev::valid_row(lvalid, i) && nw::box_ok(L)) {
        const int held = nw::knn_seed_walk(g, dir, L, max_d, K, slots);
        r = max_d;
        if (held == K) {
            const double fk = slots.far(K - 1);
            r = fmin(max_d, fk + (nw::margin(g, L) + 64.0 * DBL_EPSILON * fk));
        }
    }
    radius[i] = r;
    const double m = 64.0 * DBL_EPSILON * (g.scale + fabs(b.x) + fabs(b.y) + fabs(b.z) + fabs(b.w) + r);
    const double gr = r + m;
    grown[i] = make_double4(b.x - gr, b.y - gr, b.z + gr, b.w + gr);  // (NaN radius or NaN box: a NaN box, no candidates)
}

// Step 4.  Row i's candidates are one run of cand_l: where it begins and ends (rows without candidates keep the zeros of the memset).
__global__ __launch_bounds__(256) void knn_span_kernel(const uint32_t* __restrict__ cand_l, int64_t n_cand, int32_t* __restrict__ row_begin,
                                                       int32_t* __restrict__ row_end) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const uint32_t l = cand_l[c];
    if (c == 0 || cand_l[c - 1] != l) row_begin[l] = (int32_t)c;
    if (c == n_cand - 1 || cand_l[c + 1] != l) row_end[l] = (int32_t)c + 1;
}

struct KnnSel {
    const uint32_t* cand_r;
    const double* dist;
    const double* radius;
    const int32_t *row_begin, *row_end;
    uint8_t *rank, *hit;
    int k;
    uint32_t self_delta;  // left_row_base with GPK_KNN_EXCLUDE_SELF
    bool exclude_self;
};

// the high word of candidate c's key, BAD_KEY for a candidate that is not eligible (d + 0.0: a -0.0 becomes +0.0)
__device__ __forceinline__ unsigned long long knn_key_hi(const KnnSel& q, uint32_t row, double r_l, int c) {
    const double d = q.dist[c];
    const bool ok = d <= r_l && !(q.exclude_self && q.cand_r[c] == row + q.self_delta);  // (false for a NaN on either side)
    return ok ? (unsigned long long)__double_as_longlong(d + 0.0) : BAD_KEY;
}
__device__ __forceinline__ bool knn_key_less(unsigned long long ah, uint32_t al, unsigned long long bh, uint32_t bl) {
    return ah < bh || (ah == bh && al < bl);
}
__device__ __forceinline__ void knn_store_rank(const KnnSel& q, int c, bool eligible, int rank) {
    const bool h = eligible && rank < q.k;
    q.rank[c] = h ? (uint8_t)rank : NO_RANK;
    q.hit[c] = h ? 1 : 0;
}

__global__ __launch_bounds__(256) void knn_select_wave_kernel(KnnSel q, int64_t n, uint32_t* __restrict__ list, uint32_t* __restrict__ n_list) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int c0 = q.row_begin[i], cnt = q.row_end[i] - c0;
    if (cnt == 0) return;
    if (cnt > 64) {
        if (lane == 0) list[atomicAdd(n_list, 1u)] = (uint32_t)i;
        return;
    }
    unsigned long long hi = BAD_KEY;
    uint32_t lo = 0xFFFFFFFFu;
    if (lane < cnt) {
        hi = knn_key_hi(q, (uint32_t)i, q.radius[i], c0 + lane);
        lo = q.cand_r[c0 + lane];
    }
    const uint32_t hi0 = (uint32_t)hi, hi1 = (uint32_t)(hi >> 32);
    int rank = 0;
    for (int j = 0; j < cnt; ++j) {
        const unsigned long long oh = ((unsigned long long)(uint32_t)__shfl((int)hi1, j) << 32) | (uint32_t)__shfl((int)hi0, j);
        const uint32_t ol = (uint32_t)__shfl((int)lo, j);
        rank += knn_key_less(oh, ol, hi, lo) ? 1 : 0;
    }
    if (lane < cnt) knn_store_rank(q, c0 + lane, hi != BAD_KEY, rank);
}

// digit `pass` (0: the most significant byte) of the 96-bit key hi:lo, and whether the key agrees with the prefix on the bytes above it
__device__ __forceinline__ unsigned knn_digit(unsigned long long hi, uint32_t lo, int pass) {
    return pass < 8 ? (unsigned)(hi >> (56 - 8 * pass)) & 255u : (lo >> (24 - 8 * (pass - 8))) & 255u;
}
__device__ __forceinline__ bool knn_prefix_match(unsigned long long hi, uint32_t lo, unsigned long long phi, uint32_t plo, int pass) {
    if (pass == 0) return true;
    if (pass < 8) return (hi >> (64 - 8 * pass)) == (phi >> (64 - 8 * pass));
    if (hi != phi) return false;
    return pass == 8 || (lo >> (32 - 8 * (pass - 8))) == (plo >> (32 - 8 * (pass - 8)));
}

__global__ __launch_bounds__(256) void knn_select_list_kernel(KnnSel q, const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_list) {
    __shared__ unsigned long long s_hi[KNN_LDS_KEYS];
    __shared__ uint32_t s_lo[KNN_LDS_KEYS];
    __shared__ int s_c[GPK_KNN_MAX_K];
    __shared__ uint32_t s_hist[256];
    __shared__ unsigned long long s_phi;
    __shared__ uint32_t s_plo, s_want, s_n;
    const int tid = threadIdx.x;
    const uint32_t total = *n_list;
    for (uint32_t t = blockIdx.x; t < total; t += gridDim.x) {
        const uint32_t i = list[t];
        const int c0 = q.row_begin[i], cnt = q.row_end[i] - c0;
        const double r_l = q.radius[i];
        if (cnt <= KNN_LDS_KEYS) {
            for (int j = tid; j < cnt; j += 256) {
                s_hi[j] = knn_key_hi(q, i, r_l, c0 + j);
                s_lo[j] = q.cand_r[c0 + j];
            }
            __syncthreads();
            for (int j = tid; j < cnt; j += 256) {
                const unsigned long long hi = s_hi[j];
                const uint32_t lo = s_lo[j];
                int rank = 0;
                if (hi != BAD_KEY)
                    for (int o = 0; o < cnt; ++o) rank += knn_key_less(s_hi[o], s_lo[o], hi, lo) ? 1 : 0;
                knn_store_rank(q, c0 + j, hi != BAD_KEY, rank);
            }
            __syncthreads();
            continue;
        }
        // the key of rank k - 1 among the eligible ones, byte by byte from the top; all of them when there are at most k
        if (tid == 0) s_phi = 0, s_plo = 0, s_want = (uint32_t)(q.k - 1), s_n = 0;
        bool all = false;
        for (int pass = 0; pass < 12 && !all; ++pass) {
            s_hist[tid] = 0;
            __syncthreads();
            const unsigned long long phi = s_phi;
            const uint32_t plo = s_plo;
            for (int j = tid; j < cnt; j += 256) {
                const unsigned long long hi = knn_key_hi(q, i, r_l, c0 + j);
                if (hi == BAD_KEY) continue;
                const uint32_t lo = q.cand_r[c0 + j];
                if (knn_prefix_match(hi, lo, phi, plo, pass)) atomicAdd(&s_hist[knn_digit(hi, lo, pass)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t want = s_want, below = 0;
                int dgt = 0;
                while (dgt < 255 && below + s_hist[dgt] <= want) below += s_hist[dgt++];
                if (pass == 0) {  // (the first histogram holds every eligible key)
                    uint32_t m = 0;
                    for (int b = 0; b < 256; ++b) m += s_hist[b];
                    if (m <= (uint32_t)q.k) s_n = 0xFFFFFFFFu;
                }
                s_want = want - below;
                if (pass < 8)
                    s_phi |= (unsigned long long)dgt << (56 - 8 * pass);
                else
                    s_plo |= (uint32_t)dgt << (24 - 8 * (pass - 8));
            }
            __syncthreads();
            all = s_n == 0xFFFFFFFFu;
        }
        __syncthreads();
        if (tid == 0) s_n = 0;
        __syncthreads();
        const unsigned long long thi = all ? BAD_KEY - 1 : s_phi;
        const uint32_t tlo = all ? 0xFFFFFFFFu : s_plo;
        for (int j = tid; j < cnt; j += 256) {
            const unsigned long long hi = knn_key_hi(q, i, r_l, c0 + j);
            const uint32_t lo = q.cand_r[c0 + j];
            const bool keep = hi != BAD_KEY && !knn_key_less(thi, tlo, hi, lo);
            uint32_t at = 0xFFFFFFFFu;
            if (keep) at = atomicAdd(&s_n, 1u);
            if (at < (uint32_t)GPK_KNN_MAX_K)
                s_hi[at] = hi, s_lo[at] = lo, s_c[at] = c0 + j;
            else
                knn_store_rank(q, c0 + j, false, 0);
        }
        __syncthreads();
        const int kept = (int)(s_n < (uint32_t)GPK_KNN_MAX_K ? s_n : (uint32_t)GPK_KNN_MAX_K);
        if (tid < kept) {
            int rank = 0;
            for (int o = 0; o < kept; ++o) rank += knn_key_less(s_hi[o], s_lo[o], s_hi[tid], s_lo[tid]) ? 1 : 0;
            knn_store_rank(q, s_c[tid], true, rank);
        }
        __syncthreads();
    }
}

// Step 5.
__global__ __launch_bounds__(256) void knn_emit_kernel(const uint32_t* __restrict__ cand_l, const uint32_t* __restrict__ cand_r,
                                                       const double* __restrict__ dist, const uint8_t* __restrict__ rank, int64_t n_cand,
                                                       const int32_t* __restrict__ offsets, uint32_t left_base, uint2* __restrict__ pairs,
                                                       double* __restrict__ out_dist, int64_t capacity) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const uint8_t rk = rank[c];
    if (rk == NO_RANK) return;
    const uint32_t l = cand_l[c];
    const int64_t o = (int64_t)offsets[l] + rk;
    if (o >= capacity) return;
    pairs[o] = make_uint2(left_base + l, cand_r[c]);
    if (out_dist) out_dist[o] = dist[c] + 0.0;
}

struct KnnCtx {
    PayloadCtx p;  // (p.payload_out: the distances were asked for)
    double max_d;
    int k;
    bool exclude_self, pair_kernels;
    uint32_t left_row_base;
    const double4 *lbox, *rbox;  // set by knn_boxes
    // per left row, one block allocated by the entry point
    double* radius;
    int32_t *row_begin, *row_end;
    uint32_t *list, *n_list;
    // the candidate arrays of the refine, for the emit
    const uint32_t *cand_l, *cand_r;
    const double* dist;
    const uint8_t* rank;
    int32_t n_cand;
};

inline dim3 per_element(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// steps 1-2
int32_t knn_boxes(PayloadCtx* ctx, const gpk_index* right_index, const double4* own, double4* grown, int64_t n, hipStream_t s) {
    KnnCtx& cx = *(KnnCtx*)ctx;
    cx.lbox = own;
    cx.rbox = right_index->v.bbox;
    const GridParams& h = right_index->host_grid;
    const nw::Grid g = nw::make_grid(h.x0, h.y0, h.inv_w, h.inv_h, h.gx, h.gy);
    const KnnDir dir{right_index->v.bbox, right_index->v.cell_off, right_index->v.items, cx.p.right->d.validity};
    const int K = cx.k + (cx.exclude_self ? 1 : 0);
    const size_t lds = (size_t)K * KNN_WALK_LANES * (sizeof(double) + sizeof(uint32_t));
    GPK_LAUNCH("gpk_knn_walk", knn_walk_kernel, dim3((unsigned)((n + KNN_WALK_LANES - 1) / KNN_WALK_LANES)), dim3(KNN_WALK_LANES), lds, s, g, dir, own,
               cx.p.left->d.validity, n, cx.max_d, K, cx.radius, grown);
    return GPK_OK;
}

// steps 3-4.  Scratch: 256 bytes of counters (word 0: listed candidates of the distance kernels), dist[n_cand] (the payload's place),
// the distance kernels' list [n_cand], rank[n_cand].
int32_t knn_refine(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit, unsigned long long* stats,
                   hipStream_t s) {
    KnnCtx& cx = *(KnnCtx*)ctx;
    char* p = (char*)scratch;
    uint32_t* n_large = (uint32_t*)p;
    p += 256;
    double* dist = (double*)p;
    p += sizeof(double) * (size_t)n_cand;
    uint32_t* large = (uint32_t*)p;
    p += sizeof(uint32_t) * (size_t)n_cand;
    uint8_t* rank = (uint8_t*)p;
    const RowCands cs{cand_l, cand_r, (int64_t)n_cand, cx.lbox, cx.rbox, cx.radius, hit, dist, stats, "gpk_knn_refine", "gpk_knn_refine_large"};
    GPK_TRY(refine_row_candidates("knn_join", cx.p.left, cx.p.right, cs, cx.pair_kernels ? large : nullptr, n_large, s));
    const int64_t n = cx.p.left->d.n_geoms;
    GPK_HIP(hipMemsetAsync(cx.row_begin, 0, 2 * align256(sizeof(int32_t) * (size_t)n) + 256, s));  // row_begin, row_end, n_list
    GPK_LAUNCH("gpk_knn_span", knn_span_kernel, per_element(n_cand), dim3(256), 0, s, cand_l, (int64_t)n_cand, cx.row_begin, cx.row_end);
    const KnnSel q{cand_r, dist, cx.radius, cx.row_begin, cx.row_end, rank, hit, cx.k, cx.left_row_base, cx.exclude_self};
    GPK_LAUNCH("gpk_knn_select_wave", knn_select_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, q, n, cx.list, cx.n_list);
    GPK_LAUNCH("gpk_knn_select_list", knn_select_list_kernel, dim3(KNN_LIST_BLOCKS), dim3(256), 0, s, q, (const uint32_t*)cx.list,
               (const uint32_t*)cx.n_list);
    cx.cand_l = cand_l, cx.cand_r = cand_r, cx.dist = dist, cx.rank = rank, cx.n_cand = n_cand;
    return GPK_OK;
}

// step 5: over the pairs bbox_join emitted in candidate order
int32_t knn_emitted(void* ctx, const int32_t* offsets, uint32_t left_row_base, uint32_t* pairs, int64_t pair_capacity, hipStream_t s) {
    const KnnCtx& cx = *(const KnnCtx*)ctx;
    if (cx.n_cand <= 0) return GPK_OK;
    GPK_LAUNCH("gpk_knn_emit", knn_emit_kernel, per_element(cx.n_cand), dim3(256), 0, s, cx.cand_l, cx.cand_r, cx.dist, cx.rank, (int64_t)cx.n_cand, offsets,
               left_row_base, (uint2*)pairs, (double*)cx.p.payload_out, pair_capacity);
    return GPK_OK;
}

bool knn_family(int32_t t) {
    return t == GPK_GEOM_POINT || t == GPK_GEOM_MULTIPOINT || t == GPK_GEOM_LINESTRING || t == GPK_GEOM_MULTILINESTRING || t == GPK_GEOM_POLYGON ||
           t == GPK_GEOM_MULTIPOLYGON;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_knn_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t k, double max_distance,
                                uint32_t flags, uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist,
                                int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (k < 1 || k > GPK_KNN_MAX_K) return fail(GPK_ERR_INVALID_ARGUMENT, "knn_join: k must be in 1 .. %d, got %d", GPK_KNN_MAX_K, k);
    if (!(max_distance >= 0.0)) return fail(GPK_ERR_INVALID_ARGUMENT, "knn_join: max_distance must be >= 0 (INFINITY: no limit), got %g", max_distance);
    if (flags & ~GPK_KNN_EXCLUDE_SELF) return fail(GPK_ERR_INVALID_ARGUMENT, "knn_join: unknown flags 0x%x", flags);
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    if (!knn_family(left->d.type) || !knn_family(right->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "knn_join: unsupported geometry types %d, %d", left->d.type, right->d.type);
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "knn_join"));
    KnnCtx cx{};
    cx.p = PayloadCtx{left, right, "gpk_knn_emit", sizeof(double), nullptr};
    cx.max_d = max_distance;
    cx.k = k;
    cx.exclude_self = (flags & GPK_KNN_EXCLUDE_SELF) != 0;
    cx.left_row_base = left_row_base;
    cx.pair_kernels = left->d.type != GPK_GEOM_POINT && right->d.type != GPK_GEOM_POINT;
    // (behind the payload's 8 bytes, when distances were asked for: the distances of a call without them, the list, the rank)
    const PayloadJoin join{"knn_join", &cx.p, knn_refine, sizeof(double) + sizeof(uint32_t) + sizeof(uint8_t), knn_boxes, knn_emitted};

    // the per-row state lives in one block from the device cache (payload_join's arenas are carved by its own stages); the empty cases
    // never reach the hooks
    const int64_t n = left->d.n_geoms;
    char* block = nullptr;
    if (n > 0 && n <= (int64_t)INT32_MAX && right->d.n_geoms > 0) {
        GPK_TRY(require_device());
        const size_t f64 = align256(sizeof(double) * (size_t)n), u32 = align256(sizeof(uint32_t) * (size_t)n);
        const hipError_t e = cached_malloc((void**)&block, f64 + 3 * u32 + 256);
        if (e != hipSuccess) return fail(GPK_ERR_OOM, "knn_join: %s", hipGetErrorString(e));
        char* p = block;
        cx.radius = (double*)p, p += f64;
        cx.list = (uint32_t*)p, p += u32;
        cx.row_begin = (int32_t*)p, p += u32;  // (row_begin, row_end and n_list are zeroed by one memset)
        cx.row_end = (int32_t*)p, p += u32;
        cx.n_list = (uint32_t*)p;
    }
    const int32_t rc = payload_join(join, right_index, left_row_base, out_counts, out_pairs, out_dist, pair_capacity, n_pairs, out_space, stream);
    if (block) {
        (void)hipStreamSynchronize((hipStream_t)stream);  // (an error return may leave kernels that read the block in flight)
        cached_free(block);
    }
    return rc;
}
