// gpk_distance.h — point -> geometry Euclidean distance, G lanes cooperating on one geometry.
//   geoseries.rs:141-146,248-251 (intended impl ops::distance::euclidean_distance) — geo 0.27 euclidean_distance.rs +
//   geo-types private_utils.rs.
// Shared by the row-wise distance (gpk_rowwise.hip) and the nearest-neighbour join (gpk_nearest.hip): both evaluate a pair
// with the same functions, the same group size and the same lane order, so a pair's distance is the same double in both.
#pragma once

#include <cfloat>

#include "gpk_device.h"
#include "gpk_frac.h"

namespace gpk {

// ---- per-segment pieces -----------------------------------------------------------------------------
// geo-types private_utils::line_segment_distance, evaluated as a SQUARED distance kept as a fraction
// num / den, so that the per-segment work has no division and no hypot (both cost tens of f64
// instructions on the vector unit and made this kernel VALU-bound):
//     degenerate segment or r <= 0     -> |p - s|^2 / 1
//     r >= 1                           -> |p - e|^2 / 1
//     otherwise                        -> cross^2 / |e - s|^2          (upstream: |cross / d2| * hypot(dx, dy))
// r = dot / d2 is compared with 0 and 1 through dot <= 0 and dot >= d2 (same sign; at r ~ 1 the two
// formulas agree to O((1-r)^2)).  Fractions are compared by cross-multiplication; one divide + sqrt per
// row at the end.  Results agree with the upstream expression to a few ulps, inside the 1e-9 contract.
// (Frac and frac_less: gpk_frac.h, shared with the host)
__device__ __forceinline__ double frac_sqrt(const Frac& f) { return f.num == INFINITY ? DBL_MAX : sqrt(f.num / f.den); }

__device__ __forceinline__ Frac segment_dist2(double px, double py, double sx, double sy, double ex, double ey, double& cross_out,
                                              double& dxdy_out) {
    const double dx = ex - sx, dy = ey - sy, qx = px - sx, qy = py - sy;
    const double d2 = dx * dx + dy * dy;
    const double dot = qx * dx + qy * dy;
    const double cross = qx * dy - qy * dx;  // == -((sy - py) * dx - (sx - px) * dy)
    cross_out = cross;
    dxdy_out = dx * dy;
    if (d2 == 0.0 || dot <= 0.0) return Frac{qx * qx + qy * qy, 1.0};
    if (dot >= d2) {
        const double rx = px - ex, ry = py - ey;
        return Frac{rx * rx + ry * ry, 1.0};
    }
    return Frac{cross * cross, d2};
}

// geo-types private_utils::line_string_contains_point, one segment (tolerance f64::EPSILON on |tx - ty|).
// tx - ty == cross / (dx * dy) up to ~3 ulps of O(1) quantities, so the two divisions are only needed when
// |cross| <= 8 eps |dx dy|; everywhere else the upstream predicate is certainly false.  Inside that band the
// upstream expression is evaluated verbatim, so the zero / non-zero outcome of `distance` is exact.
__device__ __forceinline__ bool segment_contains_eps(double px, double py, double sx, double sy, double ex, double ey, double cross,
                                                     double dxdy) {
    const double dx = ex - sx, dy = ey - sy;
    if (dx == 0.0 && dy == 0.0) return px == sx && py == sy;
    if (dy == 0.0) {
        if (py != sy) return false;
        const double t = (px - sx) / dx;
        return 0.0 <= t && t <= 1.0;
    }
    if (dx == 0.0) {
        if (px != sx) return false;
        const double t = (py - sy) / dy;
        return 0.0 <= t && t <= 1.0;
    }
    if (fabs(cross) > 1.7763568394002505e-15 * fabs(dxdy)) return false;  // 8 * 2^-52
    const double tx = (px - sx) / dx, ty = (py - sy) / dy;
    return fabs(tx - ty) <= DBL_EPSILON && 0.0 <= tx && tx <= 1.0;
}

template <int G>
__device__ __forceinline__ double gmin(double v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
template <int G>
__device__ __forceinline__ Frac gmin_frac(Frac v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const Frac w{__shfl_xor(v.num, o, 64), __shfl_xor(v.den, o, 64)};
        if (frac_less(w, v)) v = w;
    }
    return v;
}
// the group's largest fraction (gpk_hausdorff.hip: the max of the lanes' minima)
template <int G>
__device__ __forceinline__ Frac gmax_frac(Frac v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const Frac w{__shfl_xor(v.num, o, 64), __shfl_xor(v.den, o, 64)};
        if (frac_less(v, w)) v = w;
    }
    return v;
}
template <int G>
__device__ __forceinline__ int gsum(int v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int G>
__device__ __forceinline__ int gor(int v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// One coordinate sequence against one point, G lanes cooperating.
struct SeqAcc {
    Frac dmin;      // min line_segment_distance, squared, as a fraction
    int wn;         // winding number (rings)
    int on_ring;    // coordinate_position boundary hit
    int eps_hit;    // line_string_contains_point (vertex equality or eps-collinear)
};
template <int G, bool WANT_DIST, bool WANT_POS>
__device__ __forceinline__ SeqAcc scan_sequence(const double2* __restrict__ xy, int c0, int c1, double px, double py,
                                                int lane) {
    SeqAcc a{Frac{INFINITY, 1.0}, 0, 0, 0};
    const int n = c1 - c0;
    if (n == 1) {
        const double2 p = xy[c0];
        const int eq = p.x == px && p.y == py;
        a.on_ring = eq;
        a.eps_hit = eq;
    }
    for (int i = c0 + lane; i + 1 < c1; i += G) {
        const double2 s = xy[i], e = xy[i + 1];
        if (WANT_POS) {
            int wn = 0;
            a.on_ring |= (int)dev::ring_edge(s.x, s.y, e.x, e.y, px, py, wn);
            a.wn += wn;
        }
        if (WANT_DIST) {
            double cross, dxdy;
            const Frac d = segment_dist2(px, py, s.x, s.y, e.x, e.y, cross, dxdy);
            if (frac_less(d, a.dmin)) a.dmin = d;
            a.eps_hit |= (int)((s.x == px && s.y == py) || (e.x == px && e.y == py) ||
                               segment_contains_eps(px, py, s.x, s.y, e.x, e.y, cross, dxdy));
        }
    }
    if (WANT_DIST) {
        a.dmin = gmin_frac<G>(a.dmin);
        a.eps_hit = gor<G>(a.eps_hit);
    }
    if (WANT_POS) {
        a.wn = gsum<G>(a.wn);
        a.on_ring = gor<G>(a.on_ring);
    }
    return a;
}
__device__ __forceinline__ int pos_of(const SeqAcc& a, int n) {
    if (n == 0) return dev::POS_OUTSIDE;
    if (a.on_ring) return dev::POS_BOUNDARY;
    return a.wn == 0 ? dev::POS_OUTSIDE : dev::POS_INSIDE;
}

// point_line_string_euclidean_distance
template <int G>
__device__ __forceinline__ double point_linestring_distance(const double2* xy, int c0, int c1, double px, double py,
                                                            int lane) {
    if (c1 == c0) return 0.0;
    const SeqAcc a = scan_sequence<G, true, false>(xy, c0, c1, px, py, lane);
    return a.eps_hit ? 0.0 : frac_sqrt(a.dmin);
}

// EuclideanDistance<Point, Polygon>: 0 if the polygon intersects the point (or its exterior is empty);
// else min over holes (as linestrings) and exterior segments.  Also returns the polygon position.
template <int G, bool WANT_DIST>
__device__ __forceinline__ double point_polygon(const DevGeo& b, int r0, int r1, double px, double py, int lane,
                                                int* pos_out) {
    *pos_out = dev::POS_OUTSIDE;
    if (r1 <= r0) return 0.0;
    const int e0 = b.ring_off[r0], e1 = b.ring_off[r0 + 1];
    if (e1 == e0) return 0.0;
    const SeqAcc ext = scan_sequence<G, WANT_DIST, true>(b.xy, e0, e1, px, py, lane);
    int pos = pos_of(ext, e1 - e0);
    double dh = DBL_MAX;
    bool resolved = pos != dev::POS_INSIDE;  // Outside / Boundary: holes do not change the position
    for (int r = r0 + 1; r < r1; ++r) {
        const int h0 = b.ring_off[r], h1 = b.ring_off[r + 1];
        if (!WANT_DIST && resolved) break;
        const SeqAcc h = scan_sequence<G, WANT_DIST, true>(b.xy, h0, h1, px, py, lane);
        if (!resolved) {
            const int ph = pos_of(h, h1 - h0);
            if (ph == dev::POS_BOUNDARY) {
                pos = dev::POS_BOUNDARY;
                resolved = true;
            } else if (ph == dev::POS_INSIDE) {
                pos = dev::POS_OUTSIDE;
                resolved = true;
            }
        }
        if (WANT_DIST) {
            const double d = (h1 == h0 || h.eps_hit) ? 0.0 : frac_sqrt(h.dmin);
            dh = d < dh ? d : dh;
        }
    }
    *pos_out = pos;
    if (!WANT_DIST) return 0.0;
    if (pos != dev::POS_OUTSIDE) return 0.0;
    const double de = frac_sqrt(ext.dmin);
    return dh < de ? dh : de;
}

// distance from one point to row j of b
// KIND selects the right-side geometry family at compile time (one instantiation per family keeps the hot
// kernel free of the other families' code and registers); KIND < 0 = decide at run time.
constexpr int KIND_ANY = -1;
template <int G, int KIND = KIND_ANY>
__device__ __forceinline__ double point_geom_distance(const DevGeo& b, int64_t j, double px, double py, int lane) {
    switch (KIND == KIND_ANY ? b.type : KIND) {
    case GPK_GEOM_POINT: {
        const double2 q = b.xy[j];
        return hypot(px - q.x, py - q.y);
    }
    case GPK_GEOM_MULTIPOINT: {
        double m = DBL_MAX;
        for (int i = b.geom_off[j] + lane; i < b.geom_off[j + 1]; i += G) {
            const double2 q = b.xy[i];
            const double d = hypot(px - q.x, py - q.y);
            m = d < m ? d : m;
        }
        return gmin<G>(m);
    }
    case GPK_GEOM_LINESTRING:
        return point_linestring_distance<G>(b.xy, b.geom_off[j], b.geom_off[j + 1], px, py, lane);
    case GPK_GEOM_MULTILINESTRING: {
        double m = DBL_MAX;
        for (int l = b.geom_off[j]; l < b.geom_off[j + 1]; ++l) {
            const double d = point_linestring_distance<G>(b.xy, b.ring_off[l], b.ring_off[l + 1], px, py, lane);
            m = d < m ? d : m;
        }
        return m;
    }
    default: {
        int p0, p1;
        dev::geom_parts(b, j, p0, p1);
        double m = DBL_MAX;
        for (int p = p0; p < p1; ++p) {
            int r0, r1, pos;
            dev::part_rings(b, p, r0, r1);
            const double d = point_polygon<G, true>(b, r0, r1, px, py, lane, &pos);
            m = d < m ? d : m;
        }
        return m;
    }
    }
}

// lanes per row of the row-wise distance (and of the nearest join): ~8 segments per lane from the mean vertex count of the
// non-point side, then rounded to the instantiated group sizes 1 / 8 / 32.  The lane order of a row's segments — hence the
// reduction order and the bits of its result — follows from G.
static inline int pick_group_rows(const DevGeo& g) {
    const double mean = g.n_geoms > 0 ? (double)g.n_coords / (double)g.n_geoms : 1.0;
    int G = 1;
    while (G < 64 && G * 2 * 8 <= mean) G <<= 1;  // ~8 segments per lane: short reductions, >= 64 B contiguous per group
    return G;
}
static inline int distance_group_size(const DevGeo& other) {
    int G = other.type == GPK_GEOM_POINT ? 1 : pick_group_rows(other);
    return G <= 1 ? 1 : (G <= 8 ? 8 : 32);  // instantiated group sizes
}

}  // namespace gpk
