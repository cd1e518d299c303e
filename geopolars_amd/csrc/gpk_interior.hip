// gpk_interior.hip — gpk_representative_point over the rules of gpk_interior.h.  Contract: include/geopolars_hip.h.
//
// Two launches a call (three for lineal and puntal columns: gpk_centroid runs first).  The first gives G lanes to every row
// (G = 4 or 16 from the column's mean coordinate count) and finishes the rows of at most INT_BLOCK_COORDS coordinates whose members
// have at most INT_SLICE crossings each; every other row is put on a list.  The second has one work-group per listed row (a
// grid-stride loop over the list, whose length stays on the device).  Both run the same member routine over a context that supplies
// the reductions: DPP row operations for a lane group, wave shuffles and LDS for a work-group.
#include "gpk_device.h"
#include "gpk_interior.h"
#include "gpk_pairdist.h"

namespace gpk {

namespace {

using ip::NO_RANK;

// ---- reductions: G lanes of a wave, or the whole work-group -------------------------------------------------------------------------
template <int G>
struct GroupCtx {
    static constexpr int T = G;
    int lane;
    __device__ __forceinline__ double dmin(double v) const { return dev::group_min<G>(v); }
    __device__ __forceinline__ double dmax(double v) const { return dev::group_max<G>(v); }
    __device__ __forceinline__ int imin(int v) const {
        return dev::group_allreduce<G>(v, [](int a, int b) { return a < b ? a : b; });
    }
    __device__ __forceinline__ int ior(int v) const { return dev::group_or<G>(v); }
};
struct BlockCtx {
    static constexpr int T = ip::INT_BLOCK_THREADS;
    static constexpr int W = T / 64;
    int lane;
    double* dslot;  // LDS, W doubles
    int* islot;     // LDS, one int
    __device__ __forceinline__ double dmin(double v) const {
        v = dev::wave_min(v);
        if ((lane & 63) == 0) dslot[lane >> 6] = v;
        __syncthreads();
        double r = dslot[0];
        for (int w = 1; w < W; ++w) r = fmin(r, dslot[w]);
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ double dmax(double v) const {
        v = dev::wave_max(v);
        if ((lane & 63) == 0) dslot[lane >> 6] = v;
        __syncthreads();
        double r = dslot[0];
        for (int w = 1; w < W; ++w) r = fmax(r, dslot[w]);
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ int imin(int v) const {
        if (lane == 0) *islot = NO_RANK;
        __syncthreads();
        if (v != NO_RANK) atomicMin(islot, v);
        __syncthreads();
        const int r = *islot;
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ int ior(int v) const {
        if (lane == 0) *islot = 0;
        __syncthreads();
        if (v) atomicOr(islot, v);
        __syncthreads();
        const int r = *islot;
        __syncthreads();
        return r;
    }
};

__device__ __forceinline__ bool finite2(double2 p) { return fabs(p.x) < INFINITY && fabs(p.y) < INFINITY; }  // (false for NaN)

// is every coordinate of [c0, c1) finite
template <class Ctx>
__device__ __forceinline__ bool range_finite(const double2* __restrict__ xy, int c0, int c1, const Ctx& cx) {
    int bad = 0;
    for (int c = c0 + cx.lane; c < c1; c += Ctx::T) bad |= finite2(xy[c]) ? 0 : 1;
    return cx.ior(bad) == 0;
}

// the scan line of the member whose coordinates are [c0, c1): box, then the ordinates next to its centre (two passes; the second
// one finds the coordinates in cache)
template <class Ctx>
__device__ __forceinline__ double member_scan(const double2* __restrict__ xy, int c0, int c1, const Ctx& cx) {
    double miny = INFINITY, maxy = -INFINITY;
    for (int c = c0 + cx.lane; c < c1; c += Ctx::T) {
        const double y = xy[c].y;
        miny = fmin(miny, y);
        maxy = fmax(maxy, y);
    }
    miny = cx.dmin(miny);
    maxy = cx.dmax(maxy);
    const double centre = ip::centre_y(miny, maxy);
    double lo = miny, hi = maxy;
    for (int c = c0 + cx.lane; c < c1; c += Ctx::T) ip::scan_update(xy[c].y, centre, lo, hi);
    return ip::scan_y(cx.dmax(lo), cx.dmin(hi));
}

// the widest section of the lanes' proposals: the widest, the lowest rank among equals (the same value on every lane)
template <class Ctx>
__device__ __forceinline__ ip::Section best_section(const ip::Section& mine, const Ctx& cx) {
    const double w = cx.dmax(mine.rank != NO_RANK ? mine.width : 0.0);
    const int rank = cx.imin(mine.rank != NO_RANK && mine.width == w ? mine.rank : NO_RANK);
    if (rank == NO_RANK) return ip::no_section();
    const double x = cx.dmax(mine.rank == rank ? mine.x : -INFINITY);  // (one lane holds the section of that rank)
    return ip::Section{w, x, rank};
}

// the members of a polygonal row
struct PolyRow {
    int p0, p1;  // parts
    int c0, c1;  // coordinates
};
__device__ __forceinline__ PolyRow poly_row(const DevGeo& g, int64_t i) {
    PolyRow r;
    dev::geom_parts(g, i, r.p0, r.p1);
    int r0, r1, q0, q1;
    r.c0 = r.c1 = 0;
    if (r.p1 > r.p0) {
        dev::part_rings(g, r.p0, r0, r1);
        dev::part_rings(g, r.p1 - 1, q0, q1);
        r.c0 = g.ring_off[r0];
        r.c1 = g.ring_off[q1];
    }
    return r;
}
// the rings [r0, r1) of part p; false: the member is empty (no ring, or an empty shell)
__device__ __forceinline__ bool member_rings(const DevGeo& g, int p, int& r0, int& r1) {
    dev::part_rings(g, p, r0, r1);
    return r1 > r0 && g.ring_off[r0 + 1] > g.ring_off[r0];
}

// ---- G lanes per row ----------------------------------------------------------------------------------------------------------------
// The crossings of the member's rings [r0, r1) into the group's slice, in storage order (a ballot compacts the lanes' finds).  Returns
// their number, which may exceed INT_SLICE: the slice then holds the first INT_SLICE of them and the row goes to the work-group.
template <int G>
__device__ __forceinline__ int collect_group(const DevGeo& g, int r0, int r1, double scan, int lane, double* __restrict__ sx, int* __restrict__ se) {
    const int gbase = (int)(threadIdx.x & 63) & ~(G - 1);
    const unsigned long long gmask = (1ull << G) - 1ull;
    int k = 0;
    for (int r = r0; r < r1; ++r) {
        const int a = g.ring_off[r], b = g.ring_off[r + 1];
        for (int base = a; base + 1 < b; base += G) {
            const int c = base + lane;
            bool keep = false;
            double x = 0.0;
            if (c + 1 < b) {
                const double2 p = g.xy[c], q = g.xy[c + 1];
                if (ip::edge_counts(p.y, q.y, scan)) {
                    keep = true;
                    x = ip::crossing_x(p.x, p.y, q.x, q.y, scan);
                }
            }
            const unsigned long long mine = (__ballot(keep) >> gbase) & gmask;
            const int pos = k + __popcll(mine & ((1ull << lane) - 1ull));
            if (keep && pos < ip::INT_SLICE) {
                sx[pos] = x;
                se[pos] = c;
            }
            k += __popcll(mine);
        }
    }
    return k;
}

__device__ __forceinline__ void group_lds_sync() {  // the lanes of a group sit in one wave: a compiler-level fence orders the LDS traffic
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G>
__global__ __launch_bounds__(256) void interior_poly_rows_kernel(DevGeo g, int64_t n, int32_t* __restrict__ big, double2* __restrict__ out_xy,
                                                                 uint8_t* __restrict__ out_valid, double* __restrict__ out_width) {
    __shared__ double slice_x[256 / G][ip::INT_SLICE];
    __shared__ int slice_e[256 / G][ip::INT_SLICE];
    const GroupCtx<G> cx{(int)(threadIdx.x & (G - 1))};
    double* sx = slice_x[threadIdx.x / G];
    int* se = slice_e[threadIdx.x / G];
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += groups) {
        ip::RowPoint pt{NAN, NAN, NAN};
        bool ok = false;
        if (dev::valid_row(g.validity, i)) {
            const PolyRow row = poly_row(g, i);
            if (row.c1 - row.c0 > ip::INT_BLOCK_COORDS) {
                if (cx.lane == 0) big[1 + atomicAdd(big, 1)] = (int32_t)i;
                continue;
            }
            bool queued = false;
            if (row.c1 > row.c0 && range_finite(g.xy, row.c0, row.c1, cx)) {
                for (int p = row.p0; p < row.p1 && !queued; ++p) {
                    int r0, r1;
                    if (!member_rings(g, p, r0, r1)) continue;
                    if (!ok) {  // the fallback: the first coordinate of the first member that counts
                        const double2 f = g.xy[g.ring_off[r0]];
                        pt = ip::RowPoint{0.0, f.x, f.y};
                        ok = true;
                    }
                    const double scan = member_scan(g.xy, g.ring_off[r0], g.ring_off[r1], cx);
                    const int k = collect_group<G>(g, r0, r1, scan, cx.lane, sx, se);
                    if (k > ip::INT_SLICE) {
                        queued = true;  // (group-uniform: k is)
                        break;
                    }
                    group_lds_sync();
                    ip::Section mine = ip::no_section();
                    for (int j = cx.lane; j < k; j += G) {
                        const double x = sx[j];
                        const int e = se[j];
                        ip::Ranked rk = ip::ranked_start();
                        for (int o = 0; o < k; ++o) ip::ranked_see(rk, x, e, sx[o], se[o]);
                        if (!(rk.rank & 1) && rk.has_succ) ip::section_propose(mine, x, rk.succ_x, rk.rank);
                    }
                    __builtin_amdgcn_wave_barrier();  // the slice may be overwritten after this point
                    ip::member_fold(pt, best_section(mine, cx), scan);
                }
            }
            if (queued) {
                if (cx.lane == 0) big[1 + atomicAdd(big, 1)] = (int32_t)i;
                continue;
            }
        }
        if (cx.lane == 0) {
            out_xy[i] = ok ? make_double2(pt.x, pt.y) : make_double2(NAN, NAN);
            if (out_valid) out_valid[i] = ok ? 1 : 0;
            if (out_width) out_width[i] = ok ? pt.width : NAN;
        }
    }
}

// ---- a work-group per listed row ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ip::INT_BLOCK_THREADS) void interior_poly_big_kernel(DevGeo g, const int32_t* __restrict__ big, double2* __restrict__ out_xy,
                                                                                  uint8_t* __restrict__ out_valid, double* __restrict__ out_width) {
    __shared__ double list_x[ip::INT_LDS_CROSSINGS];
    __shared__ int list_e[ip::INT_LDS_CROSSINGS];
    __shared__ double dslot[BlockCtx::W];
    __shared__ int islot, count;
    const int tid = threadIdx.x;
    const BlockCtx cx{tid, dslot, &islot};
    const int n_big = big[0];
    for (int q = blockIdx.x; q < n_big; q += gridDim.x) {
        const int64_t i = big[1 + q];
        const PolyRow row = poly_row(g, i);
        ip::RowPoint pt{NAN, NAN, NAN};
        bool ok = false;
        if (row.c1 > row.c0 && range_finite(g.xy, row.c0, row.c1, cx)) {
            for (int p = row.p0; p < row.p1; ++p) {
                int r0, r1;
                if (!member_rings(g, p, r0, r1)) continue;
                const int m0 = g.ring_off[r0], m1 = g.ring_off[r1];
                if (!ok) {
                    const double2 f = g.xy[m0];
                    pt = ip::RowPoint{0.0, f.x, f.y};
                    ok = true;
                }
                const double scan = member_scan(g.xy, m0, m1, cx);
                if (tid == 0) count = 0;
                __syncthreads();
                for (int c = m0 + tid; c + 1 < m1; c += BlockCtx::T) {
                    const double2 a = g.xy[c], b = g.xy[c + 1];
                    if (!ip::edge_counts(a.y, b.y, scan)) continue;
                    if (c + 1 == g.ring_off[seq_of(g.ring_off, r0, r1, c) + 1]) continue;  // (c ends its ring: no edge)
                    const int pos = atomicAdd(&count, 1);
                    if (pos < ip::INT_LDS_CROSSINGS) {
                        list_x[pos] = ip::crossing_x(a.x, a.y, b.x, b.y, scan);
                        list_e[pos] = c;
                    }
                }
                __syncthreads();
                const int k = count;
                ip::Section mine = ip::no_section();
                if (k <= ip::INT_LDS_CROSSINGS) {
                    int n2 = 2;
                    while (n2 < k) n2 <<= 1;
                    for (int j = k + tid; j < n2; j += BlockCtx::T) {
                        list_x[j] = INFINITY;
                        list_e[j] = NO_RANK;
                    }
                    __syncthreads();
                    for (int size = 2; size <= n2; size <<= 1)
                        for (int stride = size >> 1; stride > 0; stride >>= 1) {
                            for (int t = tid; t < n2 / 2; t += BlockCtx::T) {
                                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                                const bool up = (lo & size) == 0;
                                const double xa = list_x[lo], xb = list_x[hi];
                                const int ea = list_e[lo], eb = list_e[hi];
                                if (ip::crossing_less(xb, eb, xa, ea) == up) {
                                    list_x[lo] = xb; list_e[lo] = eb;
                                    list_x[hi] = xa; list_e[hi] = ea;
                                }
                            }
                            __syncthreads();
                        }
                    for (int j = 2 * tid; j + 1 < k; j += 2 * BlockCtx::T) ip::section_propose(mine, list_x[j], list_x[j + 1], j);
                } else {
                    // more crossings than the list holds: rank by walking the member's edges again (gpk_interior.h)
                    for (int c = m0 + tid; c + 1 < m1; c += BlockCtx::T) {
                        const double2 a = g.xy[c], b = g.xy[c + 1];
                        if (!ip::edge_counts(a.y, b.y, scan)) continue;
                        if (c + 1 == g.ring_off[seq_of(g.ring_off, r0, r1, c) + 1]) continue;
                        const double x = ip::crossing_x(a.x, a.y, b.x, b.y, scan);
                        ip::Ranked rk = ip::ranked_start();
                        int r = r0, r_end = g.ring_off[r0 + 1];
                        for (int o = m0; o + 1 < m1; ++o) {
                            while (o >= r_end) r_end = g.ring_off[++r + 1];
                            if (o + 1 == r_end) continue;
                            const double2 u = g.xy[o], v = g.xy[o + 1];
                            if (ip::edge_counts(u.y, v.y, scan)) ip::ranked_see(rk, x, c, ip::crossing_x(u.x, u.y, v.x, v.y, scan), o);
                        }
                        if (!(rk.rank & 1) && rk.has_succ) ip::section_propose(mine, x, rk.succ_x, rk.rank);
                    }
                }
                __syncthreads();  // the list may be overwritten after this point
                ip::member_fold(pt, best_section(mine, cx), scan);
            }
        }
        if (tid == 0) {
            out_xy[i] = ok ? make_double2(pt.x, pt.y) : make_double2(NAN, NAN);
            if (out_valid) out_valid[i] = ok ? 1 : 0;
            if (out_width) out_width[i] = ok ? pt.width : NAN;
        }
    }
}

// ---- lineal and puntal rows ----------------------------------------------------------------------------------------------------------
// The candidate nearest to `cen` over the row's sequences [s0, s1) of `so` (so == nullptr: one sequence [c0, c1) of single points, every
// coordinate is a candidate).  Lines: interior vertices, the member end points when there is none.  One pass keeps both minima.
template <class Ctx>
__device__ __forceinline__ int nearest_vertex(const double2* __restrict__ xy, const int32_t* __restrict__ so, int s0, int s1, int c0, int c1, double2 cen,
                                     const Ctx& cx) {
    ip::Nearest inner = ip::no_nearest(), ends = ip::no_nearest();
    if (!so) {
        for (int c = c0 + cx.lane; c < c1; c += Ctx::T) ip::nearest_see(inner, ip::dist2(xy[c].x, xy[c].y, cen.x, cen.y), c);
    } else {
        for (int c = c0 + cx.lane; c < c1; c += Ctx::T) {
            const int s = seq_of(so, s0, s1, c);
            const bool end = c == so[s] || c + 1 == so[s + 1];
            const double d = ip::dist2(xy[c].x, xy[c].y, cen.x, cen.y);
            if (end)
                ip::nearest_see(ends, d, c);
            else
                ip::nearest_see(inner, d, c);
        }
    }
    const bool have_inner = cx.ior(inner.index != NO_RANK) != 0;
    const ip::Nearest mine = have_inner ? inner : ends;
    const double d = cx.dmin(mine.index != NO_RANK ? mine.d : INFINITY);
    return cx.imin(mine.index != NO_RANK && mine.d == d ? mine.index : NO_RANK);
}

struct VertRow {
    const int32_t* so;
    int s0, s1, c0, c1;
};
__device__ __forceinline__ VertRow vert_row(const DevGeo& g, int64_t i) {
    if (g.type == GPK_GEOM_MULTIPOINT) return VertRow{nullptr, 0, 0, g.geom_off[i], g.geom_off[i + 1]};
    if (g.type == GPK_GEOM_LINESTRING) return VertRow{g.geom_off, (int)i, (int)i + 1, g.geom_off[i], g.geom_off[i + 1]};
    const int s0 = g.geom_off[i], s1 = g.geom_off[i + 1];  // MULTILINESTRING
    return VertRow{g.ring_off, s0, s1, s1 > s0 ? g.ring_off[s0] : 0, s1 > s0 ? g.ring_off[s1] : 0};
}

template <class Ctx>
__device__ __forceinline__ void vert_row_answer(const DevGeo& g, int64_t i, const double2* __restrict__ cen, const uint8_t* __restrict__ cen_valid, const Ctx& cx,
                                       double2* __restrict__ out_xy, uint8_t* __restrict__ out_valid, double* __restrict__ out_width) {
    const VertRow r = vert_row(g, i);
    int at = NO_RANK;
    if (r.c1 > r.c0 && cen_valid[i] && range_finite(g.xy, r.c0, r.c1, cx) && finite2(cen[i]))
        at = nearest_vertex(g.xy, r.so, r.s0, r.s1, r.c0, r.c1, cen[i], cx);
    if (cx.lane == 0) {
        out_xy[i] = at != NO_RANK ? g.xy[at] : make_double2(NAN, NAN);
        if (out_valid) out_valid[i] = at != NO_RANK ? 1 : 0;
        if (out_width) out_width[i] = NAN;
    }
}

template <int G>
__global__ __launch_bounds__(256) void interior_vert_rows_kernel(DevGeo g, int64_t n, const double2* __restrict__ cen, const uint8_t* __restrict__ cen_valid,
                                                                 int32_t* __restrict__ big, double2* __restrict__ out_xy, uint8_t* __restrict__ out_valid,
                                                                 double* __restrict__ out_width) {
    const GroupCtx<G> cx{(int)(threadIdx.x & (G - 1))};
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += groups) {
        if (!dev::valid_row(g.validity, i)) {
            if (cx.lane == 0) {
                out_xy[i] = make_double2(NAN, NAN);
                if (out_valid) out_valid[i] = 0;
                if (out_width) out_width[i] = NAN;
            }
            continue;
        }
        const VertRow r = vert_row(g, i);
        if (r.c1 - r.c0 > ip::INT_BLOCK_COORDS) {
            if (cx.lane == 0) big[1 + atomicAdd(big, 1)] = (int32_t)i;
            continue;
        }
        vert_row_answer(g, i, cen, cen_valid, cx, out_xy, out_valid, out_width);
    }
}

__global__ __launch_bounds__(ip::INT_BLOCK_THREADS) void interior_vert_big_kernel(DevGeo g, const double2* __restrict__ cen, const uint8_t* __restrict__ cen_valid,
                                                                                  const int32_t* __restrict__ big, double2* __restrict__ out_xy,
                                                                                  uint8_t* __restrict__ out_valid, double* __restrict__ out_width) {
    __shared__ double dslot[BlockCtx::W];
    __shared__ int islot;
    const BlockCtx cx{(int)threadIdx.x, dslot, &islot};
    const int n_big = big[0];
    for (int q = blockIdx.x; q < n_big; q += gridDim.x) vert_row_answer(g, big[1 + q], cen, cen_valid, cx, out_xy, out_valid, out_width);
}

// POINT columns: a point answers itself
__global__ void interior_point_kernel(DevGeo g, int64_t n, double2* __restrict__ out_xy, uint8_t* __restrict__ out_valid, double* __restrict__ out_width) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double2 p = g.xy[i];
    const bool ok = dev::valid_row(g.validity, i) && finite2(p);
    out_xy[i] = ok ? p : make_double2(NAN, NAN);
    if (out_valid) out_valid[i] = ok ? 1 : 0;
    if (out_width) out_width[i] = NAN;
}

int group_size(const DevGeo& a) {
    const double m = a.n_geoms > 0 ? (double)a.n_coords / (double)a.n_geoms : 0.0;
    return m >= ip::INT_G_MEAN ? ip::INT_G_LARGE : ip::INT_G_SMALL;
}

int32_t run(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, double* out_width, int32_t out_space, hipStream_t s) {
    const DevGeo& g = a->d;
    const int64_t n = g.n_geoms;
    if (n > (int64_t)INT32_MAX - 1) return fail(GPK_ERR_INVALID_ARGUMENT, "representative_point: more than 2^31 - 2 rows");
    const bool poly = is_polygonal(g.type), point = g.type == GPK_GEOM_POINT;
    const size_t xy_bytes = sizeof(double2) * (size_t)n, w_bytes = sizeof(double) * (size_t)n;
    Scratch sc(workspace_aux(1));  // (gpk_centroid below uses workspace())
    int32_t* big;
    double2 *xy_dev, *cen = nullptr;  // cen, cen_valid: the centroids of a lineal column's rows
    uint8_t *valid_dev, *cen_valid = nullptr;
    double* width_dev;
    sc.add(big, (size_t)(n + 1));
    sc.stage(xy_dev, (double2*)out_xy, out_space, (size_t)n);
    sc.stage(valid_dev, out_valid, out_space, (size_t)n);
    sc.stage(width_dev, out_width, out_space, (size_t)n);
    if (!point && !poly) sc.add_n((size_t)n, cen, cen_valid);
    GPK_TRY(sc.commit());
    if (point) {
        GPK_LAUNCH("gpk_representative_point", interior_point_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, n, xy_dev, valid_dev, width_dev);
    } else {
        GPK_HIP(hipMemsetAsync(big, 0, sizeof(int32_t), s));
        const int G = group_size(g);
        const dim3 grid = group_grid(n, G);
        int64_t blocks = n;  // the work-group kernel: at most the rows, every row may be queued
        if (blocks > (int64_t)cu_count() * 8) blocks = (int64_t)cu_count() * 8;
        if (poly) {
            if (G == ip::INT_G_SMALL)
                GPK_LAUNCH("gpk_representative_point", (interior_poly_rows_kernel<ip::INT_G_SMALL>), grid, dim3(256), 0, s, g, n, big, xy_dev, valid_dev, width_dev);
            else
                GPK_LAUNCH("gpk_representative_point", (interior_poly_rows_kernel<ip::INT_G_LARGE>), grid, dim3(256), 0, s, g, n, big, xy_dev, valid_dev, width_dev);
            GPK_LAUNCH("gpk_representative_point_large", interior_poly_big_kernel, dim3((unsigned)blocks), dim3(ip::INT_BLOCK_THREADS), 0, s, g, big, xy_dev,
                       valid_dev, width_dev);
        } else {
            GPK_TRY(gpk_centroid(a, (double*)cen, cen_valid, GPK_MEM_DEVICE, s));
            if (G == ip::INT_G_SMALL)
                GPK_LAUNCH("gpk_representative_point", (interior_vert_rows_kernel<ip::INT_G_SMALL>), grid, dim3(256), 0, s, g, n, cen, cen_valid, big, xy_dev,
                           valid_dev, width_dev);
            else
                GPK_LAUNCH("gpk_representative_point", (interior_vert_rows_kernel<ip::INT_G_LARGE>), grid, dim3(256), 0, s, g, n, cen, cen_valid, big, xy_dev,
                           valid_dev, width_dev);
            if (g.n_coords > ip::INT_BLOCK_COORDS)  // (else no row can be on the list)
                GPK_LAUNCH("gpk_representative_point_large", interior_vert_big_kernel, dim3((unsigned)blocks), dim3(ip::INT_BLOCK_THREADS), 0, s, g, cen, cen_valid,
                           big, xy_dev, valid_dev, width_dev);
        }
    }
    if (out_valid) GPK_TRY(copy_out(out_valid, out_space, valid_dev, (size_t)n, s));
    if (out_width) GPK_TRY(copy_out(out_width, out_space, width_dev, w_bytes, s));
    return copy_out(out_xy, out_space, xy_dev, xy_bytes, s);
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_representative_point(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, double* out_width, int32_t out_space, void* stream) {
    if (!a || !out_xy) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    GPK_TRY(require_device());
    if (a->d.n_geoms == 0) return GPK_OK;
    return run(a, out_xy, out_valid, out_width, out_space, (hipStream_t)stream);
}
