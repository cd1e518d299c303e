// gpk_hausdorff.hip — row-wise discrete Hausdorff distance between two geometry columns of any of the six families
// (gpk_hausdorff_distance; the per-row rules are in gpk_hausdorff.h, the contract in include/geopolars_hip.h).
//
// Polygon interiors play no part, so the family only decides how a row's coordinate sequences are found: one kernel instance per
// lane-group size, with a run-time family switch in front of row_seqs.
//
// Schedules.  A directed pass h(L -> W) costs (samples of L) x (coordinates of W) point-segment terms:
//   hausdorff_kernel<G>       G lanes per row (G = 8 or 32, pairdist_group_size).  Lanes stride over the slots of L, G at a time, each
//                             holding the running minimum of its sample while the group walks every segment of W with uniform loads;
//                             the lane folds the minimum into its running maximum, gmax_frac joins the lanes at the end.  Then the
//                             other direction, then pick_max and one square root.  Rows above HD_LARGE_COST are appended to a list.
//   hausdorff_large_kernel    one 256-lane work-group per listed row.  Thread t owns slots t, t + 256, ... of L; the walked side is
//                             staged in LDS, PDL_CHUNK segments at a time (staged once when it fits one chunk, else again for every
//                             round of 256 samples: a sample's minimum must be complete before it meets the maximum).  The four
//                             waves' maxima are folded in a fixed order.  The list's length is read on the device: no read-back.
//                             Cost of the re-staging: with n_W > PDL_CHUNK walked segments and r = ceil(samples / 256) rounds the
//                             work-group stages r * n_W segments (a seq_of binary search each) and passes 2 r ceil(n_W / PDL_CHUNK)
//                             barriers, against 256 r n_W terms of some thirty f64 operations: one staged segment per 256 terms, at
//                             most a few per cent.  Chunks outside and rounds inside would stage n_W once, but needs every sample's
//                             running minimum kept across chunks — r fractions a thread, unbounded in registers; it is not built.
// No early exit: a group could stop walking once every lane's minimum is below the group's maximum; it is not built.
// The columns are taken in canonical order (the smaller family code first, as pair_distance_dev does) and neither the lane order of a
// directed pass nor pick_max depends on which row is called A, so H(a, b) and H(b, a) are the same double.
#include "gpk_hausdorff.h"
#include "gpk_pairdist.h"

namespace gpk {

namespace {

// the sequences of row j of any family, row_seqs (gpk_pairdist.h) behind a run-time family switch; a POINT is one sequence of one
// coordinate (none when a coordinate is NaN: an empty point)
__device__ __forceinline__ RowSeqs hd_row_seqs(const DevGeo& g, int64_t j) {
    RowSeqs r{g.xy, nullptr, 0, 0, 0, 0};
    if (g.type == GPK_GEOM_POINT) {
        const double2 p = g.xy[j];
        r.c0 = (int)j;
        r.c1 = (int)j + ((p.x == p.x && p.y == p.y) ? 1 : 0);
        return r;
    }
    int s0 = g.geom_off[j], s1 = g.geom_off[j + 1];
    if (g.type == GPK_GEOM_MULTIPOINT) {  // as row_seqs<GPK_GEOM_MULTIPOINT>: no sequence table
        r.c0 = s0;
        r.c1 = s1;
        return r;
    }
    if (g.type == GPK_GEOM_LINESTRING) {  // as row_seqs<GPK_GEOM_LINESTRING>
        r.so = g.geom_off;
        s0 = (int)j;
        s1 = (int)j + 1;
    } else {  // as row_seqs of POLYGON / MULTILINESTRING, and of MULTIPOLYGON through its parts
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
    return r;
}

// non-empty sequences of a row (its coordinates when it has no sequence table); same value on every lane of the group
template <int G>
__device__ __forceinline__ int nonempty_seqs(const RowSeqs& r, int lane) {
    if (!r.so) return r.c1 - r.c0;
    int q = 0;
    for (int s = r.s0 + lane; s < r.s1; s += G) q += r.so[s + 1] > r.so[s] ? 1 : 0;
    return gsum<G>(q);
}

__device__ __forceinline__ double2 slot_sample(const RowSeqs& l, int64_t c, int j, int k, double2 p) {
    if (j == 0) return p;
    const double2 q = l.xy[c + 1];
    return make_double2(hd::sample_coord(p.x, q.x, j, k), hd::sample_coord(p.y, q.y, j, k));
}

// h(L -> W) by G lanes: the same fraction on lane 0 of every call with the same two rows, whichever is called A
template <int G>
__device__ __forceinline__ Frac directed_group(const RowSeqs& l, const RowSeqs& w, int k, int lane) {
    const int kk = l.so ? k : 1;
    const int64_t c_end = l.c1;
    int64_t c = (int64_t)l.c0 + lane / kk;  // this lane's slot (c, j); every round moves it G slots on
    int j = lane % kk;
    int ls = l.s0;                          // this lane's sequence cursor in L
    const int64_t slots = (int64_t)(l.c1 - l.c0) * kk;
    Frac mx = hd::no_max();
    for (int64_t u0 = 0; u0 < slots; u0 += G) {
        bool active = c < c_end;
        double2 p = make_double2(0.0, 0.0);
        if (active) {
            p = l.xy[c];
            if (l.so) {
                while (l.so[ls + 1] <= c) ++ls;
                if (j > 0 && c + 1 == l.so[ls + 1]) active = false;  // no slot after a sequence's last vertex
            }
            if (active) p = slot_sample(l, c, j, kk, p);
        }
        Frac mn = hd::no_min();
        int ws = w.s0, wend = w.so ? w.so[w.s0 + 1] : 0;  // the walk's sequence cursor (group-uniform)
        double2 p0 = w.xy[w.c0];
        for (int i = w.c0; i < w.c1; ++i) {
            const double2 nx = i + 1 < w.c1 ? w.xy[i + 1] : p0;
            if (w.so) {
                while (wend <= i) wend = w.so[++ws + 1];
            }
            const double2 p1 = (w.so && i + 1 < wend) ? nx : p0;
            if (active) hd::see_min(mn, pair_seg_dist2(p.x, p.y, p0.x, p0.y, p1.x, p1.y));
            p0 = nx;
        }
        if (active) hd::see_max(mx, mn);
        j += G;
        c += j / kk;
        j %= kk;
    }
    return gmax_frac<G>(mx);
}

// h(L -> W) by a 256-lane work-group; valid on thread 0.  Ends with a barrier: the LDS can be reused at once.
__device__ __forceinline__ Frac directed_workgroup(const RowSeqs& l, const RowSeqs& w, int k, PairLargeLds& lds) {
    const int tid = threadIdx.x, wave = tid >> 6, lane64 = tid & 63;
    const int kk = l.so ? k : 1;
    const int64_t slots = (int64_t)(l.c1 - l.c0) * kk;
    const int nw = w.c1 - w.c0;
    const bool one_chunk = nw <= PDL_CHUNK;
    Frac mx = hd::no_max();
    for (int64_t u0 = 0; u0 < slots; u0 += 256) {
        const int64_t u = u0 + tid;
        bool active = u < slots;
        double2 p = make_double2(0.0, 0.0);
        if (active) {
            const int64_t c = (int64_t)l.c0 + u / kk;
            const int j = (int)(u % kk);
            p = l.xy[c];
            if (l.so && j > 0 && c + 1 == l.so[seq_of(l.so, l.s0, l.s1, (int)c) + 1]) active = false;
            if (active) p = slot_sample(l, c, j, kk, p);
        }
        Frac mn = hd::no_min();
        for (int ch = 0; ch < nw; ch += PDL_CHUNK) {
            const int len = nw - ch < PDL_CHUNK ? nw - ch : PDL_CHUNK;
            if (!one_chunk || u0 == 0) {
                __syncthreads();  // the previous chunk is no longer read
                for (int t = tid; t < len; t += 256) {
                    const int cw = w.c0 + ch + t;
                    const double2 p0 = w.xy[cw];
                    const double2 p1 = w.so ? seg_end(w, seq_of(w.so, w.s0, w.s1, cw), cw, p0) : p0;
                    lds.seg[t] = make_double4(p0.x, p0.y, p1.x, p1.y);
                }
                __syncthreads();
            }
            if (active) {
                for (int t = 0; t < len; ++t) {
                    const double4 s = lds.seg[t];
                    hd::see_min(mn, pair_seg_dist2(p.x, p.y, s.x, s.y, s.z, s.w));
                }
            }
        }
        if (active) hd::see_max(mx, mn);
    }
    const Frac m = gmax_frac<64>(mx);
    if (lane64 == 0) {
        lds.num[wave] = m.num;
        lds.den[wave] = m.den;
    }
    __syncthreads();
    Frac best{lds.num[0], lds.den[0]};  // the four waves in a fixed order
    for (int v = 1; v < 4; ++v) hd::see_max(best, Frac{lds.num[v], lds.den[v]});
    __syncthreads();
    return best;
}

__device__ __forceinline__ void hd_pair_rows(const uint32_t* __restrict__ rows, bool swapped, int64_t i, int64_t& ia, int64_t& ib) {
    const int64_t j = rows ? (int64_t)rows[i] : i;
    ia = swapped ? j : i;
    ib = swapped ? i : j;
}

// One lane group per row and no row loop: nothing is carried from row to row.  (ga, gb): the columns in canonical order; `swapped`:
// gb is the caller's left column, so the row map indexes ga.
template <int G>
__global__ __launch_bounds__(256) void hausdorff_kernel(DevGeo ga, DevGeo gb, const uint32_t* __restrict__ rows, bool swapped, int64_t n, int k,
                                                        double* __restrict__ out, uint32_t* __restrict__ large_rows, uint32_t* __restrict__ n_large) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (i >= n) return;
    int64_t ia, ib;
    hd_pair_rows(rows, swapped, i, ia, ib);
    double d = NAN;
    if (dev::row_ok(ga, ia) && dev::row_ok(gb, ib)) {
        const RowSeqs a = hd_row_seqs(ga, ia), b = hd_row_seqs(gb, ib);
        const int64_t na = a.c1 - a.c0, nb = b.c1 - b.c0;
        if (na > 0 && nb > 0) {
            const int64_t sa = hd::sample_count(na, nonempty_seqs<G>(a, lane), k, a.so != nullptr);
            const int64_t sb = hd::sample_count(nb, nonempty_seqs<G>(b, lane), k, b.so != nullptr);
            if (hd::cost(sa, na, sb, nb) > hd::HD_LARGE_COST) {
                if (lane == 0) large_rows[atomicAdd(n_large, 1u)] = (uint32_t)i;
                return;
            }
            const Frac hab = directed_group<G>(a, b, k, lane);
            const Frac hba = directed_group<G>(b, a, k, lane);
            d = hd::result(hd::pick_max(hab, hba));
        }
    }
    if (lane == 0) out[i] = d;
}

__global__ __launch_bounds__(256) void hausdorff_large_kernel(DevGeo ga, DevGeo gb, const uint32_t* __restrict__ rows, bool swapped, int k,
                                                              const uint32_t* __restrict__ large_rows, const uint32_t* __restrict__ n_large,
                                                              double* __restrict__ out) {
    __shared__ PairLargeLds lds;
    const uint32_t count = *n_large;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const int64_t i = large_rows[e];
        int64_t ia, ib;
        hd_pair_rows(rows, swapped, i, ia, ib);
        const RowSeqs a = hd_row_seqs(ga, ia), b = hd_row_seqs(gb, ib);
        const Frac hab = directed_workgroup(a, b, k, lds);
        const Frac hba = directed_workgroup(b, a, k, lds);
        if (threadIdx.x == 0) out[i] = hd::result(hd::pick_max(hab, hba));
    }
}

constexpr unsigned HD_LIST_BLOCKS = 1024;  // four work-groups a compute unit on the 256-CU part this library targets

int32_t hausdorff_dev(const DevGeo& a, const DevGeo& b, const uint32_t* rows, int64_t n, int k, double* out, uint32_t* large_rows, uint32_t* n_large,
                      hipStream_t s) {
    GPK_HIP(hipMemsetAsync(n_large, 0, sizeof(uint32_t), s));
    const bool swapped = a.type > b.type;
    const DevGeo& ga = swapped ? b : a;
    const DevGeo& gb = swapped ? a : b;
    const int G = pairdist_group_size(ga, gb);
    // exactly one lane group per row: ceil(n / (256 / G)) blocks, no cap and no row loop in the kernel
    const int64_t per_block = 256 / G;
    const dim3 grid((unsigned)((n + per_block - 1) / per_block)), block(256);
    if (G == 8)
        GPK_LAUNCH("gpk_hausdorff", (hausdorff_kernel<8>), grid, block, 0, s, ga, gb, rows, swapped, n, k, out, large_rows, n_large);
    else
        GPK_LAUNCH("gpk_hausdorff", (hausdorff_kernel<32>), grid, block, 0, s, ga, gb, rows, swapped, n, k, out, large_rows, n_large);
    // the listed rows: a fixed grid of HD_LIST_BLOCKS work-groups (the device's CU count is not asked) that loops over the list and reads
    // its length on the device; tests/test_gpu_hausdorff.py lists more rows than that, so the loop runs past its first pass
    GPK_LAUNCH("gpk_hausdorff_large", hausdorff_large_kernel, dim3(HD_LIST_BLOCKS), block, 0, s, ga, gb, rows, swapped, k, (const uint32_t*)large_rows,
               (const uint32_t*)n_large, out);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_hausdorff_distance(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, int32_t subdivisions, double* out,
                                          int32_t out_space, void* stream) {
    if (!a || !b || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (subdivisions < 1 || subdivisions > hd::MAX_SUBDIVISIONS)
        return fail(GPK_ERR_INVALID_ARGUMENT, "hausdorff_distance: subdivisions must be within 1 .. %d (found %d)", hd::MAX_SUBDIVISIONS, (int)subdivisions);
    if (!b_rows && a->d.n_geoms != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "hausdorff_distance: row counts differ (%lld vs %lld)", (long long)a->d.n_geoms, (long long)b->d.n_geoms);
    const int64_t n = a->d.n_geoms;
    if (n > (int64_t)INT32_MAX - 1) return fail(GPK_ERR_INVALID_ARGUMENT, "hausdorff_distance: more than 2^31 - 2 rows");
    GPK_TRY(require_device());
    if (n == 0) return GPK_OK;
    hipStream_t s = (hipStream_t)stream;
    Scratch sc(workspace());
    double* out_dev;
    const uint32_t* rows_dev;
    uint32_t *large_rows, *n_large;
    sc.stage(out_dev, out, out_space, (size_t)n);
    sc.stage_in(rows_dev, b_rows, out_space, (size_t)n);
    sc.add(large_rows, (size_t)n);
    sc.add(n_large, 1);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    GPK_TRY(hausdorff_dev(a->d, b->d, rows_dev, n, (int)subdivisions, out_dev, large_rows, n_large, s));
    return sc.copy_back(s);
}
