// gpk_overlay.h — how much two geometries share: the area of A ∩ B for two polygonal rows and the length of L ∩ P for a lineal and a
// polygonal row (gpk_intersection_measure, include/geopolars_hip.h).  Neither builds the intersection geometry:
// both are sums of independent (edge, edge) terms, with no output offsets and no noding.
//
// Oriented edges.  The edges of every ring of a polygonal row are taken in the direction that puts the geometry's interior on their
// left: the stored order when (ring.ccw > 0) != is_hole, reversed otherwise (the a_left rule of pp::overlap_bits).  Zero-length edges
// are dropped.
//
// Inside fraction.  For a segment e = (a -> b) and a polygonal geometry Q with oriented edges f = (c -> d)
//   tau_Q(e) = sum over f of  sgn_f * mu(e, f)
//   sgn_f    = +1 if d.x < c.x (Q's interior lies below f), -1 if d.x > c.x; a vertical f contributes nothing
//   mu(e, f) = length of { t in [0, 1] : p(t).x in the x-range of f and p(t) below the line of f }
// — the winding number of an upward ray, integrated along e.  It is linear in the edges of Q, so every (e, f) pair stands alone.  The
// x-range clips t to one interval [t0, t1]; inside it "below" changes at most once, and the exact signs orient(c, d, a), orient(c, d, b)
// say how: equal signs give t1 - t0 or 0, opposite signs put the change at t* = |da| / (|da| + |db|) (floating determinants, clamped to
// the interval), one zero sign lets the other decide.  An f whose y-range lies wholly above e's is above without an orientation call,
// one wholly below contributes nothing.
//
// Area.    area(A ∩ B) = 1/2 sum_{e in A} cross(a - o, b - o) tau_B(e)  +  1/2 sum_{f in B} cross(c - o, d - o) tau_A(f)
// Green's theorem over the boundary of A ∩ B, which consists of the pieces of A's rings inside B and of B's rings inside A.  o is a
// pair-local origin, the centre of the intersection of the two rows' boxes: every term is then at most (box diagonal)^2, whatever the
// placement — without it the terms lose every digit at georeferenced magnitudes.
//
// Ties (shared edges, a polygon filling a hole, equal polygons).  They are decided as for ONE fixed infinitesimal translation of B by
// (+eps1, +eps2), eps1 << eps2, the same in both sums; the area is continuous under translation, so the limit is the exact area and
// overlaps need no case of their own:
//                                              points of A against edges of B      points of B against edges of A
//   x-range (matters for a vertical e only)    (min, max]                          [min, max)
//   both orientations zero (collinear)         below                               above
//
// Length.  length(L ∩ P) = sum over the segments pq of L of |pq| * ( tau_P(pq) + kappa(pq) ),  P closed
// tau_P with the points-of-A rules; kappa adds back the pieces that run along a ring edge and that the translation left outside: for
// every f collinear with the segment, the length of the shared t-range when f runs rightward (d.x > c.x) or is vertical and runs
// downward (d.y < c.y).  A line that runs over the same stretch twice counts it twice.
//
// The pair terms are plain C++ (no HIP type, no intrinsic) and take the orientation predicate as a template argument: the device
// passes the exact cont::orient, a host program its own (tests/overlay_host_driver.cpp runs them with __int128).  The group routines
// on top are device code.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define GPK_OV_FN __host__ __device__ inline
#else
#define GPK_OV_FN inline
#endif

namespace gpk {
namespace ov {

struct P2 {
    double x, y;
};

GPK_OV_FN double cross_at(P2 a, P2 b, P2 o) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

// sgn_f * mu(e, f) for e = (a -> b), a != b, and the oriented edge f = (c -> d), c != d.  `points_of_a`: e belongs to the first
// geometry (or to the line) and f to the second — the left column of the tie table; false: the right column.
// orient(p, q, r): the exact sign of cross(q - p, r - p).
template <class Orient>
GPK_OV_FN double inside_term(P2 a, P2 b, P2 c, P2 d, bool points_of_a, Orient orient) {
    if (c.x == d.x) return 0.0;
    const bool leftward = d.x < c.x;
    const double sgn = leftward ? 1.0 : -1.0;
    const double flo = leftward ? d.x : c.x, fhi = leftward ? c.x : d.x;
    double t0 = 0.0, t1 = 1.0;
    if (a.x == b.x) {
        if (!(points_of_a ? (a.x > flo && a.x <= fhi) : (a.x >= flo && a.x < fhi))) return 0.0;
    } else {
        const double inv = 1.0 / (b.x - a.x);
        const double u = (flo - a.x) * inv, v = (fhi - a.x) * inv;
        t0 = fmax(0.0, fmin(u, v));
        t1 = fmin(1.0, fmax(u, v));
        if (!(t1 > t0)) return 0.0;
    }
    const double len = t1 - t0;
    if (fmin(c.y, d.y) > fmax(a.y, b.y)) return sgn * len;
    if (fmax(c.y, d.y) < fmin(a.y, b.y)) return 0.0;
    int sa = orient(c, d, a), sb = orient(c, d, b);  // > 0: below the line of f, once f is read left to right
    if (!leftward) {
        sa = -sa;
        sb = -sb;
    }
    if (sa == 0 && sb == 0) return points_of_a ? sgn * len : 0.0;
    if (sa >= 0 && sb >= 0) return sgn * len;
    if (sa <= 0 && sb <= 0) return 0.0;
    const double ex = d.x - c.x, ey = d.y - c.y;
    const double da = fabs(ex * (a.y - c.y) - ey * (a.x - c.x)), db = fabs(ex * (b.y - c.y) - ey * (b.x - c.x));
    const double ts = fmin(t1, fmax(t0, da + db > 0.0 ? da / (da + db) : 0.5));
    return sgn * (sa > 0 ? ts - t0 : t1 - ts);
}

// kappa's term: the share of the segment p -> q (p != q) that runs along the oriented ring edge f = (c -> d), c != d, when f is one of
// the edges whose pieces the tie translation leaves outside
template <class Orient>
GPK_OV_FN double along_term(P2 p, P2 q, P2 c, P2 d, Orient orient) {
    if (!(d.x > c.x || (d.x == c.x && d.y < c.y))) return 0.0;
    if (fmax(c.x, d.x) < fmin(p.x, q.x) || fmin(c.x, d.x) > fmax(p.x, q.x) || fmax(c.y, d.y) < fmin(p.y, q.y) || fmin(c.y, d.y) > fmax(p.y, q.y))
        return 0.0;
    if (orient(c, d, p) != 0 || orient(c, d, q) != 0) return 0.0;
    const bool by_x = p.x != q.x;
    const double p1 = by_x ? p.x : p.y, inv = 1.0 / ((by_x ? q.x : q.y) - p1);
    const double u = ((by_x ? c.x : c.y) - p1) * inv, v = ((by_x ? d.x : d.y) - p1) * inv;
    const double lo = fmax(0.0, fmin(u, v)), hi = fmin(1.0, fmax(u, v));
    return hi > lo ? hi - lo : 0.0;
}

// the pair-local origin: the centre of the intersection of two boxes (x0, y0, x1, y1) that are not apart
GPK_OV_FN P2 local_origin(double ax0, double ay0, double ax1, double ay1, double bx0, double by0, double bx1, double by1) {
    return P2{0.5 * fmax(ax0, bx0) + 0.5 * fmin(ax1, bx1), 0.5 * fmax(ay0, by0) + 0.5 * fmin(ay1, by1)};
}

}  // namespace ov
}  // namespace gpk

#if defined(__HIPCC__)
// ---- the device group routines ------------------------------------------------------------------------------------------------------
// G lanes take one pair, exactly as in gpk_polyrel.h: the outer edge is the same on all lanes, the lanes stride the other geometry's
// edges, ring by ring over all rings of all parts.  A lane keeps one running sum and the group adds the G sums with the fixed butterfly
// of dev::group_sum, so a pair's value depends on G alone, never on the launch that computed it: the join returns bit for bit what the
// row-wise call returns.  An outer edge whose box strictly misses the box of the other row's shells is skipped (its tau is exactly
// zero; strict, so a shared edge on the box border is still seen); rows whose boxes are strictly apart give exactly 0.0; results are
// clamped to >= 0.  G: pp::relation_group_size for two polygonal columns, lp::relation_group_size for lines.  There is no work-group
// path for huge rows, the limit gpk_polyrel.hip states.
//
// Rows (lp::polygon_row_ok and the line rule of gpk_lineline.h): NaN when either row is null or out of range, has no non-empty member /
// no coordinate, a ring that fails cont::ring_init, or — a line — a NaN or infinite coordinate.  Invalid polygons: the value is
// unspecified, the routine terminates.
#include "gpk_polyrel.h"

namespace gpk {
namespace ov {

struct DevOrient {
    __device__ __forceinline__ int operator()(P2 a, P2 b, P2 c) const { return dev::orient2d(a.x, a.y, b.x, b.y, c.x, c.y); }
};
__device__ __forceinline__ P2 p2(double2 v) { return P2{v.x, v.y}; }
__device__ __forceinline__ bool boxes_apart(double4 a, double4 b) { return a.z < b.x || a.x > b.z || a.w < b.y || a.y > b.w; }
__device__ __forceinline__ bool edge_misses(P2 a, P2 b, double4 box) {
    return fmax(a.x, b.x) < box.x || fmin(a.x, b.x) > box.z || fmax(a.y, b.y) < box.y || fmin(a.y, b.y) > box.w;
}

// this lane's share of  sum_{e in X} cross(a - o, b - o) tau_Y(e)  for the usable rows X[x0, x1), Y[y0, y1)
template <int G>
__device__ inline double green_lane_sum(const DevGeo& X, int x0, int x1, const DevGeo& Y, int y0, int y1, double4 box_y, P2 o, bool x_is_a, int lane) {
    double acc = 0.0;
    for (int px = x0; px < x1; ++px) {
        int xr0, xr1;
        if (!lp::part_of(X, px, xr0, xr1)) continue;
        for (int rx = xr0; rx < xr1; ++rx) {
            const int xc0 = X.ring_off[rx], xn = X.ring_off[rx + 1] - xc0;
            if (xn == 0) continue;
            cont::Ring RX;
            (void)cont::ring_init<G>(RX, X.xy + xc0, xn, lane);
            const bool x_left = (RX.ccw > 0) != (rx > xr0);
            for (int py = y0; py < y1; ++py) {
                int yr0, yr1;
                if (!lp::part_of(Y, py, yr0, yr1)) continue;
                for (int ry = yr0; ry < yr1; ++ry) {
                    const int yc0 = Y.ring_off[ry], yn = Y.ring_off[ry + 1] - yc0;
                    if (yn == 0) continue;
                    cont::Ring RY;
                    (void)cont::ring_init<G>(RY, Y.xy + yc0, yn, lane);
                    const bool y_left = (RY.ccw > 0) != (ry > yr0);
                    for (int i = 0; i < RX.m; ++i) {
                        const P2 a = p2(RX.v[x_left ? i : i + 1]), b = p2(RX.v[x_left ? i + 1 : i]);
                        if ((a.x == b.x && a.y == b.y) || edge_misses(a, b, box_y)) continue;
                        double tau = 0.0;
                        for (int j = lane; j < RY.m; j += G) {
                            const P2 c = p2(RY.v[y_left ? j : j + 1]), d = p2(RY.v[y_left ? j + 1 : j]);
                            if (c.x == d.x && c.y == d.y) continue;
                            tau += inside_term(a, b, c, d, x_is_a, DevOrient{});
                        }
                        acc += cross_at(a, b, o) * tau;
                    }
                }
            }
        }
    }
    return acc;
}

// area(a[i] ∩ b[j]), both POLYGON | MULTIPOLYGON; rows out of range behave like null rows.  Same value on every lane of the group.
template <int G>
__device__ inline double intersection_area_group(const DevGeo& a, int64_t i, const DevGeo& b, int64_t j, int lane) {
    if (!dev::row_ok(a, i) || !dev::row_ok(b, j)) return NAN;
    int a0, a1, b0, b1;
    dev::geom_parts(a, i, a0, a1);
    dev::geom_parts(b, j, b0, b1);
    double4 box_a, box_b;
    if (!lp::polygon_row_ok<G>(a, a0, a1, lane, box_a) || !lp::polygon_row_ok<G>(b, b0, b1, lane, box_b)) return NAN;
    if (boxes_apart(box_a, box_b)) return 0.0;
    const P2 o = local_origin(box_a.x, box_a.y, box_a.z, box_a.w, box_b.x, box_b.y, box_b.z, box_b.w);
    const double mine = green_lane_sum<G>(a, a0, a1, b, b0, b1, box_b, o, true, lane) + green_lane_sum<G>(b, b0, b1, a, a0, a1, box_a, o, false, lane);
    return fmax(0.0, 0.5 * dev::group_sum<G>(mine));
}

// length(lines[i] ∩ polys[j]), LINESTRING | MULTILINESTRING against POLYGON | MULTIPOLYGON.  Same value on every lane of the group.
template <int G>
__device__ inline double intersection_length_group(const DevGeo& lines, int64_t i, const DevGeo& polys, int64_t j, int lane) {
    if (!dev::row_ok(lines, i) || !dev::row_ok(polys, j)) return NAN;
    const RowSeqs l = lp::line_seqs(lines, i);
    if (l.c1 <= l.c0) return NAN;
    double4 box_l;
    {
        int bad = 0;
        double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
        for (int c = l.c0 + lane; c < l.c1; c += G) {
            const double2 v = l.xy[c];
            bad |= !(fabs(v.x) < INFINITY) | !(fabs(v.y) < INFINITY);  // NaN or infinite
            mnx = fmin(mnx, v.x); mny = fmin(mny, v.y); mxx = fmax(mxx, v.x); mxy = fmax(mxy, v.y);
        }
        if (dev::group_or<G>(bad)) return NAN;
        box_l = make_double4(dev::group_min<G>(mnx), dev::group_min<G>(mny), dev::group_max<G>(mxx), dev::group_max<G>(mxy));
    }
    int p0, p1;
    dev::geom_parts(polys, j, p0, p1);
    double4 box;
    if (!lp::polygon_row_ok<G>(polys, p0, p1, lane, box)) return NAN;
    if (boxes_apart(box_l, box)) return 0.0;
    double acc = 0.0;
    for (int pt = p0; pt < p1; ++pt) {
        int r0, r1;
        if (!lp::part_of(polys, pt, r0, r1)) continue;
        for (int r = r0; r < r1; ++r) {
            const int rc0 = polys.ring_off[r], rn = polys.ring_off[r + 1] - rc0;
            if (rn == 0) continue;
            cont::Ring R;
            (void)cont::ring_init<G>(R, polys.xy + rc0, rn, lane);
            const bool left = (R.ccw > 0) != (r > r0);
            for (int s = l.s0; s < l.s1; ++s) {
                for (int c = l.so[s] + 1; c < l.so[s + 1]; ++c) {
                    const P2 p = p2(l.xy[c - 1]), q = p2(l.xy[c]);
                    if ((p.x == q.x && p.y == q.y) || edge_misses(p, q, box)) continue;
                    double t = 0.0;
                    for (int k = lane; k < R.m; k += G) {
                        const P2 e = p2(R.v[left ? k : k + 1]), f = p2(R.v[left ? k + 1 : k]);
                        if (e.x == f.x && e.y == f.y) continue;
                        t += inside_term(p, q, e, f, true, DevOrient{}) + along_term(p, q, e, f, DevOrient{});
                    }
                    const double dx = q.x - p.x, dy = q.y - p.y;
                    acc += sqrt(dx * dx + dy * dy) * t;
                }
            }
        }
    }
    return fmax(0.0, dev::group_sum<G>(acc));
}

}  // namespace ov
}  // namespace gpk
#endif
