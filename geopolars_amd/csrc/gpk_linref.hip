// gpk_linref.hip — linear referencing on the device.
//   gpk_closest_point_rowwise    geo 0.27 ClosestPoint / shapely nearest_points, shortest_line: the point of B nearest to p
//   gpk_line_locate_point        geo LineLocatePoint / GeoSeries.project: the measure along a line of the point nearest to p
//   gpk_line_interpolate_point   geo LineInterpolatePoint / GeoSeries.interpolate: the point at a measure along a line
//
// Mapping: as the row-wise distance (gpk_rowwise.hip distance_kernel) — G lanes (1 / 8 / 32 from the mean vertex count of the
// non-point side) share one row, lane k takes segments k, k+G, ... so a group reads contiguous 16-byte coordinates; rows of a tile
// are walked longest first.  One instance per G and right-side family.  Locate is two passes over the row: the arg-min scan, then
// the lengths of the segments before the winner (they are in L2 from the first pass; on average half a row of square roots).
// Interpolate gives one group per line: segment lengths over consecutive chunks of G, a group prefix per chunk, then the chunk and
// lane whose cumulative end measure first reaches the distance.
#include <cfloat>

#include "gpk_device.h"
#include "gpk_distance.h"
#include "gpk_linref.h"

namespace gpk {
namespace {

__device__ __forceinline__ void store_xy(double* __restrict__ out_xy, int64_t i, double x, double y) {
    out_xy[2 * i] = x;  // (two 8-byte stores: the caller's buffer need not be 16-byte aligned)
    out_xy[2 * i + 1] = y;
}

// ---- closest point ----------------------------------------------------------------------------------------------------------
template <int G, int KIND>
__global__ __launch_bounds__(256) void closest_point_kernel(DevGeo pts, DevGeo other, const uint32_t* __restrict__ rows, double* __restrict__ out_xy,
                                                            int32_t* __restrict__ out_seg) {
    for_rows_binned<G>(pts.n_geoms, other, rows, [&](int64_t i, int64_t j, int lane) {
        const double2 p = pts.xy[i];
        double2 q = make_double2(NAN, NAN);
        int seg = -1;
        if (dev::valid_row(pts.validity, i) && dev::row_ok(other, j) && !isnan(p.x) && !isnan(p.y)) {
            if (KIND == GPK_GEOM_POINT) {
                const double2 s = other.xy[j];
                if (!isnan(s.x) && !isnan(s.y)) {  // (an empty POINT has NaN coordinates)
                    q = s;
                    seg = (int)j;
                }
            } else {
                bool inside;
                const ArgMin a = argmin_row<G, KIND>(other, j, p.x, p.y, lane, &inside);
                if (inside) {
                    q = p;
                } else if (a.idx != INT_MAX) {
                    double along;
                    q = segment_nearest(p.x, p.y, other.xy[a.idx], other.xy[a.end], &along);
                    seg = a.idx;
                }
            }
        }
        if (lane == 0) {
            store_xy(out_xy, i, q.x, q.y);
            if (out_seg) out_seg[i] = seg;
        }
    });
}

// ---- locate -------------------------------------------------------------------------------------------------------------------
template <int G, int KIND>
__global__ __launch_bounds__(256) void locate_point_kernel(DevGeo pts, DevGeo lines, const uint32_t* __restrict__ rows, int normalized,
                                                           double* __restrict__ out) {
    for_rows_binned<G>(pts.n_geoms, lines, rows, [&](int64_t i, int64_t j, int lane) {
        const double2 p = pts.xy[i];
        double m = NAN;
        if (dev::valid_row(pts.validity, i) && dev::row_ok(lines, j) && !isnan(p.x) && !isnan(p.y)) {
            bool inside;
            const ArgMin a = argmin_row<G, KIND>(lines, j, p.x, p.y, lane, &inside);
            if (a.idx != INT_MAX) {
                double before, total, along;
                measure_before<G>(lines, j, a.idx, normalized != 0, lane, &before, &total);
                segment_nearest(p.x, p.y, lines.xy[a.idx], lines.xy[a.end], &along);
                m = before + along;
                if (normalized) m = total > 0.0 ? m / total : 0.0;
            }
        }
        if (lane == 0) out[i] = m;
    });
}

// ---- interpolate ----------------------------------------------------------------------------------------------------------------
// The row's segments in storage order, G at a time, with a running measure `base` (the same bits on every lane).  With `find`: stops at
// the first segment whose cumulative end measure is >= d.  Returns the measure walked (the row's total length when nothing was hit).
struct WalkHit {
    int seg;               // start coordinate of the segment reached, -1: none
    double m0, len, cum;   // measure at its start, its length, measure at its end
    int first, last;       // first and last coordinate of the row (-1: the row has none)
};
template <int G>
__device__ __forceinline__ double walk_measure(const DevGeo& b, int64_t j, double d, bool find, int lane, WalkHit* hit) {
    const int32_t* off;
    int m0, m1;
    lineal_members(b, j, off, m0, m1);
    const int sub = ((threadIdx.x & 63) / G) * G;  // the group's first lane within the wave
    double base = 0.0;
    hit->seg = hit->first = hit->last = -1;
    for (int m = m0; m < m1; ++m) {
        const int c0 = off[m], c1 = off[m + 1];
        if (c1 == c0) continue;
        if (hit->first < 0) hit->first = c0;
        hit->last = c1 - 1;
        for (int c = c0; c + 1 < c1; c += G) {
            const int i = c + lane;
            const bool mine = i + 1 < c1;
            const double len = mine ? segment_length(b.xy[i], b.xy[i + 1]) : 0.0;
            const double pre = gprefix_f64<G>(len, lane);
            if (find) {
                const double cum = base + pre;
                const unsigned long long wave = __ballot(mine && cum >= d);
                const unsigned long long mask = G == 64 ? wave : (wave >> sub) & ((1ull << G) - 1ull);
                if (mask) {
                    const int w = __ffsll((long long)mask) - 1;
                    double excl = __shfl_up(pre, 1, G);
                    if (lane == 0) excl = 0.0;
                    hit->seg = c + w;
                    hit->m0 = __shfl(base + excl, w, G);
                    hit->len = __shfl(len, w, G);
                    hit->cum = __shfl(cum, w, G);
                    return base;
                }
            }
            base += __shfl(pre, G - 1, G);
        }
    }
    return base;
}

template <int G>
__global__ __launch_bounds__(256) void interpolate_point_kernel(DevGeo lines, const double* __restrict__ dist, int64_t dist_stride, double dist_scalar,
                                                                int normalized, double* __restrict__ out_xy, uint8_t* __restrict__ out_valid) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t n = lines.n_geoms, step = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += step) {
        double d = dist ? dist[i * dist_stride] : dist_scalar;
        double2 q = make_double2(NAN, NAN);
        int ok = 0;
        if (dev::valid_row(lines.validity, i) && !isnan(d)) {
            WalkHit h;
            if (normalized || d < 0.0) {  // the total length first: the same walk, so that the second one reaches it exactly
                const double L = walk_measure<G>(lines, i, 0.0, false, lane, &h);
                if (normalized) d *= L;
                if (d < 0.0) d += L;
                d = d < 0.0 ? 0.0 : (d > L ? L : d);
            }
            const double walked = walk_measure<G>(lines, i, d, true, lane, &h);
            if (h.first >= 0) {
                ok = 1;
                if (h.seg < 0) {  // beyond the end (or no segment at all): the last coordinate; a line without length: its first
                    q = lines.xy[walked > 0.0 ? h.last : h.first];
                } else {
                    const double2 s = lines.xy[h.seg], e = lines.xy[h.seg + 1];
                    const double t = (d - h.m0) / h.len;
                    if (d == h.cum)
                        q = e;
                    else if (!(t > 0.0))
                        q = s;
                    else if (t >= 1.0)
                        q = e;
                    else
                        q = make_double2(s.x + t * (e.x - s.x), s.y + t * (e.y - s.y));
                }
            }
        }
        if (lane == 0) {
            store_xy(out_xy, i, q.x, q.y);
            if (out_valid) out_valid[i] = (uint8_t)ok;
        }
    }
}

dim3 tile_grid(int64_t n) {
    int64_t n_tiles = (n + LINREF_TILE - 1) / LINREF_TILE;
    if (n_tiles > (int64_t)cu_count() * 16) n_tiles = (int64_t)cu_count() * 16;
    return dim3((unsigned)n_tiles);
}

#define LINREF_BY_G(LAUNCH, KK) \
    do {                        \
        if (G == 1)             \
            LAUNCH(1, KK);      \
        else if (G == 8)        \
            LAUNCH(8, KK);      \
        else                    \
            LAUNCH(32, KK);     \
    } while (0)

}  // namespace
}  // namespace gpk

using namespace gpk;

extern "C" {

int32_t gpk_closest_point_rowwise(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double* out_xy, int32_t* out_seg,
                                  int32_t out_space, void* stream) {
    if (!a || !b || !out_xy) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (a->d.type != GPK_GEOM_POINT)
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "closest_point: the first array must be POINT (found type %d)", a->d.type);
    if (!b_rows && a->d.n_geoms != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "closest_point: row counts differ (%lld vs %lld)", (long long)a->d.n_geoms, (long long)b->d.n_geoms);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = a->d.n_geoms;
    if (n == 0) return GPK_OK;
    const size_t xb = 2 * sizeof(double) * (size_t)n, sb = sizeof(int32_t) * (size_t)n;
    Scratch sc(workspace());
    const uint32_t* rows_dev;
    double* xy_dev;
    int32_t* seg_dev;
    sc.stage(xy_dev, out_xy, out_space, 2 * (size_t)n);
    sc.stage(seg_dev, out_seg, out_space, (size_t)n);
    sc.stage_in(rows_dev, b_rows, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    const int G = distance_group_size(b->d);
    const dim3 grid = tile_grid(n), block(256);
#define CP_LAUNCH(GG, KK) GPK_LAUNCH("gpk_closest_point", (closest_point_kernel<GG, KK>), grid, block, 0, s, a->d, b->d, rows_dev, xy_dev, seg_dev)
    switch (b->d.type) {
    case GPK_GEOM_POINT: CP_LAUNCH(1, GPK_GEOM_POINT); break;
    case GPK_GEOM_MULTIPOINT: LINREF_BY_G(CP_LAUNCH, GPK_GEOM_MULTIPOINT); break;
    case GPK_GEOM_LINESTRING: LINREF_BY_G(CP_LAUNCH, GPK_GEOM_LINESTRING); break;
    case GPK_GEOM_MULTILINESTRING: LINREF_BY_G(CP_LAUNCH, GPK_GEOM_MULTILINESTRING); break;
    case GPK_GEOM_POLYGON: LINREF_BY_G(CP_LAUNCH, GPK_GEOM_POLYGON); break;
    default: LINREF_BY_G(CP_LAUNCH, GPK_GEOM_MULTIPOLYGON); break;
    }
#undef CP_LAUNCH
    if (out_seg && out_space != GPK_MEM_DEVICE) GPK_HIP(hipMemcpyAsync(out_seg, seg_dev, sb, hipMemcpyDeviceToHost, s));
    return copy_out(out_xy, out_space, xy_dev, xb, s);
}

int32_t gpk_line_locate_point(const gpk_geoarray* pts, const gpk_geoarray* lines, const uint32_t* line_rows, int32_t normalized, double* out,
                              int32_t out_space, void* stream) {
    if (!pts || !lines || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (pts->d.type != GPK_GEOM_POINT || !is_lineal(lines->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "line_locate_point: POINT x LINESTRING | MULTILINESTRING (found types %d, %d)", pts->d.type,
                    lines->d.type);
    if (!line_rows && pts->d.n_geoms != lines->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_locate_point: row counts differ (%lld vs %lld)", (long long)pts->d.n_geoms,
                    (long long)lines->d.n_geoms);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = pts->d.n_geoms;
    if (n == 0) return GPK_OK;
    Scratch sc(workspace());
    const uint32_t* rows_dev;
    double* out_dev;
    sc.stage(out_dev, out, out_space, (size_t)n);
    sc.stage_in(rows_dev, line_rows, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    const int G = distance_group_size(lines->d);
    const dim3 grid = tile_grid(n), block(256);
#define LL_LAUNCH(GG, KK) \
    GPK_LAUNCH("gpk_line_locate_point", (locate_point_kernel<GG, KK>), grid, block, 0, s, pts->d, lines->d, rows_dev, (int)normalized, out_dev)
    if (lines->d.type == GPK_GEOM_LINESTRING)
        LINREF_BY_G(LL_LAUNCH, GPK_GEOM_LINESTRING);
    else
        LINREF_BY_G(LL_LAUNCH, GPK_GEOM_MULTILINESTRING);
#undef LL_LAUNCH
    return sc.copy_back(s);
}

int32_t gpk_line_interpolate_point(const gpk_geoarray* lines, const double* distances, int64_t n_distances, int32_t normalized, double* out_xy,
                                   uint8_t* out_valid, int32_t out_space, void* stream) {
    if (!lines || !distances || !out_xy) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_lineal(lines->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "line_interpolate_point: LINESTRING | MULTILINESTRING (found type %d)", lines->d.type);
    const int64_t n = lines->d.n_geoms;
    if (n_distances != 1 && n_distances != n)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_interpolate_point: %lld distances for %lld rows (1 or one per row)", (long long)n_distances,
                    (long long)n);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return GPK_OK;
    const bool host = out_space != GPK_MEM_DEVICE;
    const bool broadcast = n_distances == 1 && n != 1;
    const size_t xb = 2 * sizeof(double) * (size_t)n, vb = (size_t)n;
    // one value for every row: a host value travels as a kernel argument, a device value is read in place with stride 0
    const bool by_value = host && n_distances == 1;
    const double scalar = by_value ? distances[0] : 0.0;
    Scratch sc(workspace());
    const double* dist_dev;
    double* xy_dev;
    uint8_t* valid_dev;
    sc.stage(xy_dev, out_xy, out_space, 2 * (size_t)n);
    sc.stage(valid_dev, out_valid, out_space, (size_t)n);
    sc.stage_in(dist_dev, by_value ? nullptr : distances, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    const int64_t stride = broadcast ? 0 : 1;
    const int G = distance_group_size(lines->d);
    const dim3 grid = group_grid(n, G), block(256);  // (n > 0 here: the helper never gives an empty grid)
#define LI_LAUNCH(GG, KK) \
    GPK_LAUNCH("gpk_line_interpolate_point", (interpolate_point_kernel<GG>), grid, block, 0, s, lines->d, dist_dev, stride, scalar, (int)normalized, xy_dev, valid_dev)
    LINREF_BY_G(LI_LAUNCH, 0);
#undef LI_LAUNCH
    if (out_valid && host) GPK_HIP(hipMemcpyAsync(out_valid, valid_dev, vb, hipMemcpyDeviceToHost, s));
    return copy_out(out_xy, out_space, xy_dev, xb, s);
}

}  // extern "C"
