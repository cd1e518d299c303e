// gpk_geodesic.hip — gpk_geodesic_area / gpk_geodesic_inverse / gpk_geodesic_direct: the geodesic measures of gpk_geodesic.h over columns of
// (lon, lat) degrees on WGS84.  Contract: include/geopolars_hip.h; DESIGN.md section 4.3v has the schedule and the resource figures.
//
// Area and perimeter.  An edge costs a few thousand f64 operations for 16 bytes of input, so the schedule is flat: one lane per EDGE in
// storage order, one work-group per strip of ga::STRIP consecutive coordinates, the grid sized from the coordinate count.  Rows of any
// shape balance by construction and a wave's loads are consecutive.
//   edges   lane t of strip b owns coordinate c = b * STRIP + t: its ring by bisection of the ring offsets, the edge c -> c + 1 when c is
//           not the last coordinate of its ring.  (s12, S12, transit) go to LDS; the first lane of every run of one ring folds the run in
//           storage order.  A ring that lies inside the strip gets its record in ring_tab[ring]; a ring that crosses a strip boundary
//           leaves a partial in strip_tab: slot 1 of the strip where it begins, slot 0 of every later strip it reaches.
//   rows    one lane per row: the rings of its parts, each record from ring_tab or folded from the strip partials in strip order, the
//           reduction of gpk::geodesic::ring_area per ring, then the signed or unsigned fold.
// Every area sum is an error-free pair (gpk::geodesic::Sum2) from the lane to the row; no floating-point atomic anywhere, every fold in
// a fixed order: two calls give the same bits.
#include "gpk_common.h"
#include "gpk_device.h"
#include "gpk_geodesic.h"
#include "gpk_scratch.h"

namespace gpk {

namespace ga {

constexpr int STRIP = 256;  // coordinates a work-group: one a lane

struct Partial {  // the fold of a run of edges
    double s_hi, s_lo;  // sum of S12, an error-free pair
    double per;         // sum of s12
    int32_t transit, pad;
};

__device__ __forceinline__ bool polygonal(int32_t type) { return type == GPK_GEOM_POLYGON || type == GPK_GEOM_MULTIPOLYGON; }

// the last r in [0, n] with off[r] <= c, or -1
__device__ __forceinline__ int64_t seq_of(const int32_t* __restrict__ off, int64_t n, int64_t c) {
    int64_t lo = 0, hi = n + 1;  // first entry > c lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= c) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// (One instance: the perimeter alone runs it too.  An instance without the area series was measured and was 1.7x SLOWER than this one —
// 248 VGPRs and one wave a SIMD against 201 and two — so asking for less would have cost more.)
__global__ __launch_bounds__(STRIP) void area_edges_kernel(const double2* __restrict__ xy, const int32_t* __restrict__ ring_off, int64_t n_rings,
                                                           int64_t n_coords, Partial* __restrict__ ring_tab, Partial* __restrict__ strip_tab) {
    __shared__ double l_s12[STRIP], l_S12[STRIP];
    __shared__ int32_t l_ring[STRIP], l_tr[STRIP];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * STRIP, c = base + t;
    int64_t ring = -1;
    double s12 = 0.0, S12 = 0.0;
    int tr = 0;
    if (c < n_coords) {
        ring = seq_of(ring_off, n_rings, c);
        if (ring >= n_rings) ring = -1;  // past the last ring
        if (ring >= 0 && c + 1 < (int64_t)ring_off[ring + 1] && c + 1 < n_coords) {
            const double2 p = xy[c], q = xy[c + 1];
            const geodesic::Inverse r = geodesic::inverse<true>(p.x, p.y, q.x, q.y);
            s12 = r.s12;
            S12 = r.S12;
            tr = geodesic::transit(p.x, q.x);
        }
    }
    l_s12[t] = s12;
    l_S12[t] = S12;
    l_tr[t] = tr;
    l_ring[t] = (int32_t)ring;
    __syncthreads();
    if (ring < 0 || (t > 0 && l_ring[t - 1] == (int32_t)ring)) return;  // not the first lane of a run
    geodesic::Sum2 a{0.0, 0.0};
    double per = 0.0;
    int crossings = 0;
    for (int u = t; u < STRIP && l_ring[u] == (int32_t)ring; ++u) {
        a = geodesic::sum2_add(a, l_S12[u]);
        per += l_s12[u];
        crossings += l_tr[u];
    }
    const Partial out{a.hi, a.lo, per, crossings, 0};
    const int64_t r0 = ring_off[ring], r1 = ring_off[ring + 1];
    if (r0 >= base && r1 <= base + STRIP) ring_tab[ring] = out;
    else strip_tab[2 * (int64_t)blockIdx.x + (r0 < base ? 0 : 1)] = out;
}

__device__ inline Partial ring_record(const int32_t* __restrict__ ring_off, int64_t r, const Partial* __restrict__ ring_tab,
                                      const Partial* __restrict__ strip_tab) {
    const int64_t r0 = ring_off[r], r1 = ring_off[r + 1];
    if (r1 <= r0) return Partial{0.0, 0.0, 0.0, 0, 0};
    const int64_t first = r0 / STRIP, last = (r1 - 1) / STRIP;
    if (first == last) return ring_tab[r];
    Partial p = strip_tab[2 * first + 1];
    for (int64_t k = first + 1; k <= last; ++k) {
        const Partial q = strip_tab[2 * k];
        const geodesic::Sum2 a = geodesic::sum2_join(geodesic::Sum2{p.s_hi, p.s_lo}, geodesic::Sum2{q.s_hi, q.s_lo});
        p.s_hi = a.hi;
        p.s_lo = a.lo;
        p.per += q.per;
        p.transit += q.transit;
    }
    return p;
}

__global__ __launch_bounds__(256) void area_rows_kernel(DevGeo a, uint32_t flags, const Partial* __restrict__ ring_tab,
                                                        const Partial* __restrict__ strip_tab, double* __restrict__ out_area,
                                                        double* __restrict__ out_per) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_geoms) return;
    double area = 0.0, per = 0.0;
    if (!dev::valid_row(a.validity, g)) {
        area = per = NAN;
    } else if (polygonal(a.type)) {
        geodesic::Sum2 sum{0.0, 0.0};
        int p0, p1;
        dev::geom_parts(a, g, p0, p1);
        for (int p = p0; p < p1; ++p) {
            int q0, q1;
            dev::part_rings(a, p, q0, q1);
            for (int r = q0; r < q1; ++r) {
                const Partial rec = ring_record(a.ring_off, r, ring_tab, strip_tab);
                per += rec.per;
                if (out_area) {
                    const double v = geodesic::ring_area(geodesic::Sum2{rec.s_hi, rec.s_lo}, rec.transit);
                    sum = geodesic::sum2_add(sum, (flags & GPK_GEODESIC_AREA_SIGNED) ? v : (r == q0 ? fabs(v) : -fabs(v)));
                }
            }
        }
        area = sum.hi;
    }
    if (out_area) out_area[g] = area;
    if (out_per) out_per[g] = per;
}

// one lane per row: a[i] against b[b_rows ? b_rows[i] : i], both POINT
__global__ __launch_bounds__(256) void inverse_kernel(DevGeo a, DevGeo b, const uint32_t* __restrict__ b_rows, double* __restrict__ out_s12,
                                                      double* __restrict__ out_azi1, double* __restrict__ out_azi2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_geoms) return;
    const int64_t j = b_rows ? (int64_t)b_rows[i] : i;
    geodesic::Inverse r{NAN, NAN, NAN, NAN, NAN};
    if (dev::row_ok(a, i) && dev::row_ok(b, j)) {
        const double2 p = a.xy[i], q = b.xy[j];
        if (p.x == p.x && p.y == p.y && q.x == q.x && q.y == q.y) r = geodesic::inverse<false>(p.x, p.y, q.x, q.y);
    }
    if (out_s12) out_s12[i] = r.s12;
    if (out_azi1) out_azi1[i] = r.azi1;
    if (out_azi2) out_azi2[i] = r.azi2;
}

// one lane per row; azi1 / s12 hold one value for every row (n == 1) or one a row
__global__ __launch_bounds__(256) void direct_kernel(DevGeo a, const double* __restrict__ azi1, int64_t n_azi, const double* __restrict__ s12,
                                                     int64_t n_s12, double2* __restrict__ out_xy, double* __restrict__ out_azi2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_geoms) return;
    geodesic::Direct r{NAN, NAN, NAN};
    if (dev::valid_row(a.validity, i)) {
        const double2 p = a.xy[i];
        const double az = azi1[n_azi == 1 ? 0 : i], s = s12[n_s12 == 1 ? 0 : i];
        if (p.x == p.x && p.y == p.y && az - az == 0.0 && s - s == 0.0) r = geodesic::direct(p.x, p.y, az, s);  // (x - x: NaN for NaN and infinity)
    }
    out_xy[i] = make_double2(r.lon2, r.lat2);
    if (out_azi2) out_azi2[i] = r.azi2;
}

inline dim3 lanes_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)); }

}  // namespace ga
}  // namespace gpk

using namespace gpk;

extern "C" {

int32_t gpk_geodesic_area(const gpk_geoarray* a, uint32_t flags, double* out_area, double* out_perimeter, int32_t out_space, void* stream) {
    if (!a) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (flags & ~GPK_GEODESIC_AREA_SIGNED) return fail(GPK_ERR_INVALID_ARGUMENT, "geodesic_area: unknown flag bits 0x%x", (unsigned)flags);
    const int64_t n = a->d.n_geoms;
    if (n == 0 || (!out_area && !out_perimeter)) return GPK_OK;
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const bool poly = a->d.type == GPK_GEOM_POLYGON || a->d.type == GPK_GEOM_MULTIPOLYGON;
    const int64_t nc = poly ? a->d.n_coords : 0, n_rings = poly ? a->d.n_rings : 0;
    const int64_t strips = (nc + ga::STRIP - 1) / ga::STRIP;
    Scratch sc(workspace());
    ga::Partial *ring_tab, *strip_tab;
    double *area_dev, *per_dev;
    sc.add(ring_tab, (size_t)n_rings);
    sc.add(strip_tab, 2 * (size_t)strips);
    sc.stage(area_dev, out_area, out_space, (size_t)n);
    sc.stage(per_dev, out_perimeter, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    if (strips > 0 && n_rings > 0) {
        GPK_LAUNCH("gpk_geodesic_area_edges", ga::area_edges_kernel, dim3((unsigned)strips), dim3(ga::STRIP), 0, s, a->d.xy, a->d.ring_off, n_rings, nc,
                   ring_tab, strip_tab);
    }
    GPK_LAUNCH("gpk_geodesic_area_rows", ga::area_rows_kernel, ga::lanes_grid(n), dim3(256), 0, s, a->d, flags, (const ga::Partial*)ring_tab,
               (const ga::Partial*)strip_tab, area_dev, per_dev);
    return sc.copy_back(s);
}

int32_t gpk_geodesic_inverse(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double* out_s12, double* out_azi1,
                             double* out_azi2, int32_t out_space, void* stream) {
    if (!a || !b) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (a->d.type != GPK_GEOM_POINT || b->d.type != GPK_GEOM_POINT)
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "geodesic_inverse: both columns must be POINT (got types %d and %d)", (int)a->d.type, (int)b->d.type);
    const int64_t n = a->d.n_geoms;
    if (!b_rows && b->d.n_geoms != n)
        return fail(GPK_ERR_INVALID_ARGUMENT, "geodesic_inverse: row counts differ (%lld and %lld) and no b_rows was given", (long long)n,
                    (long long)b->d.n_geoms);
    if (n == 0 || (!out_s12 && !out_azi1 && !out_azi2)) return GPK_OK;
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    Scratch sc(workspace());
    const uint32_t* rows_dev;
    double *s12_dev, *azi1_dev, *azi2_dev;
    sc.stage_in(rows_dev, b_rows, out_space, (size_t)n);
    sc.stage(s12_dev, out_s12, out_space, (size_t)n);
    sc.stage(azi1_dev, out_azi1, out_space, (size_t)n);
    sc.stage(azi2_dev, out_azi2, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    GPK_LAUNCH("gpk_geodesic_inverse", ga::inverse_kernel, ga::lanes_grid(n), dim3(256), 0, s, a->d, b->d, rows_dev, s12_dev, azi1_dev, azi2_dev);
    return sc.copy_back(s);
}

int32_t gpk_geodesic_direct(const gpk_geoarray* a, const double* azi1, int64_t n_azi, const double* s12, int64_t n_s12, double* out_xy,
                            double* out_azi2, int32_t out_space, void* stream) {
    if (!a) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (a->d.type != GPK_GEOM_POINT) return fail(GPK_ERR_MISMATCHED_GEOMETRY, "geodesic_direct: the column must be POINT (got type %d)", (int)a->d.type);
    const int64_t n = a->d.n_geoms;
    if ((n_azi != 1 && n_azi != n) || (n_s12 != 1 && n_s12 != n))
        return fail(GPK_ERR_INVALID_ARGUMENT, "geodesic_direct: n_azi (%lld) and n_s12 (%lld) must each be 1 or the row count %lld", (long long)n_azi,
                    (long long)n_s12, (long long)n);
    if (!azi1 || !s12) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n == 0) return GPK_OK;
    if (!out_xy) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    Scratch sc(workspace());
    const double *azi_dev, *s12_dev;
    double *xy_dev, *azi2_dev;
    sc.stage_in(azi_dev, azi1, out_space, (size_t)n_azi);
    sc.stage_in(s12_dev, s12, out_space, (size_t)n_s12);
    sc.stage(xy_dev, out_xy, out_space, 2 * (size_t)n);
    sc.stage(azi2_dev, out_azi2, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    GPK_LAUNCH("gpk_geodesic_direct", ga::direct_kernel, ga::lanes_grid(n), dim3(256), 0, s, a->d, azi_dev, n_azi, s12_dev, n_s12, (double2*)xy_dev, azi2_dev);
    return sc.copy_back(s);
}

}  // extern "C"
