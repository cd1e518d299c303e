// gpk_minbound.h — the two bounding shapes of a row's convex hull: the rules of gpk_minimum_rotated_rectangle and
// gpk_minimum_bounding_circle (include/geopolars_hip.h states the contract; DESIGN.md section 4.3n the schedules).
//
// Both read the hull ring v_0 .. v_{h-1} exactly as gpk_convex_hull writes it: counter-clockwise, starting at the lexicographically
// smallest vertex, no collinear vertices, closing vertex dropped.
//
// Rectangle.  For edge i, a = v_i and d = v_{i+1} - a:
//   L2 = d . d; for every hull vertex w, u = w - a taken first, s = u . d and t = d x u; smin, smax, tmax over the hull
//   (smin <= 0 <= smax and tmax >= 0: a is among the vertices); A_i = (smax - smin) * tmax; the rectangle on edge i has area A_i / L2_i.
//   choice    the edge of least area, compared by cross-multiplication A_i * L2_j < A_j * L2_i; a later edge only when strictly
//             smaller, so equal areas on exactly representable data go to the lowest edge index.
//   corners   c0 = a + (smin / L2) d, c1 = a + (smax / L2) d, c2 = c1 + (tmax / L2) (-d_y, d_x), c3 = c0 + (tmax / L2) (-d_y, d_x);
//             the ring is c0 c1 c2 c3 c0, counter-clockwise.
//   degenerate  one distinct point: that point five times; all coordinates collinear (hull ring p q p): p q q p p.
// Circle.  Row-local coordinates p = v - v_0.  The state is a support of two or three hull vertices, the centre and the squared radius:
//   two points    centre = their midpoint ((a + b) / 2 per ordinate);
//   three points  the circumcentre on differences from the first support point a: b' = b - a, c' = c - a, D = 2 (b'_x c'_y - b'_y c'_x),
//                 centre = a + ((c'_y |b'|^2 - b'_y |c'|^2) / D, (b'_x |c'|^2 - c'_x |b'|^2) / D);
//   radius^2      the squared distance from the centre to the first support point.
//   start         v_0 and the vertex farthest from it (the lowest index among equals).
//   iteration     q = the vertex farthest from the centre (lowest index among equals); stop when it is not outside (d2 <= r2) or is a
//                 support vertex already.  Otherwise the candidates are, in this order, the two-point circles of q with each old support
//                 point, then the three-point circles of q with each pair of them; a candidate's reach is the largest squared distance
//                 from its centre to q and the old support points; the candidate of least reach wins, a later one only when strictly
//                 less (so a two-point circle wins a tie: the right triangle).  In exact arithmetic that is the smallest circle of
//                 the old support and q, the radius grows strictly and the iteration ends at the smallest circle of the hull.
//   bound         MBG_CIRCLE_ITERS iterations; when they run out the answer is the current centre with the distance to the farthest
//                 vertex as radius (a circle that still contains the row).
// Every operation is rounded on its own (the build uses -ffp-contract=off).
//
// Everything in this file is plain C++ (no HIP type, no intrinsic): the device kernels (gpk_minbound.hip) and a host program
// (tests/minbound_host_driver.cpp) run the same functions.
#pragma once

#include <cmath>

#include "../../include/geopolars_hip.h"  // MBG_CIRCLE_ITERS, the bound of the circle iteration

#if defined(__HIPCC__)
#define GPK_MB_FN __host__ __device__ __forceinline__
#else
#define GPK_MB_FN inline
#endif

namespace gpk {
namespace mb {

constexpr int MBG_G = 16;               // lanes a row in the lane-group kernel: one DPP row
constexpr int MBG_SMALL_HULL = 128;     // hulls of at most this many vertices take the lane-group kernel (the hull's own small cap)
constexpr int MBG_BIG_THREADS = 256;    // the work-group kernel
constexpr int MBG_BIG_BLOCKS = 1024;    // its grid is min(rows, MBG_BIG_BLOCKS) work-groups striding over the list
constexpr int MBG_LDS_HULL = 4096;      // hulls of at most this many vertices are staged in LDS by the work-group kernel (64 KB)
constexpr int NO_EDGE = 0x7fffffff;

// ---- rectangle ----------------------------------------------------------------------------------------------------------------------
struct Extent {
    double smin, smax, tmax;
};
GPK_MB_FN Extent extent_start() { return Extent{0.0, 0.0, 0.0}; }  // (the extent of a itself)
GPK_MB_FN double proj_s(double ax, double ay, double dx, double dy, double wx, double wy) {
    const double ux = wx - ax, uy = wy - ay;
    return ux * dx + uy * dy;
}
GPK_MB_FN double proj_t(double ax, double ay, double dx, double dy, double wx, double wy) {
    const double ux = wx - ax, uy = wy - ay;
    return dx * uy - dy * ux;
}
GPK_MB_FN void extent_see(Extent& e, double ax, double ay, double dx, double dy, double wx, double wy) {
    const double s = proj_s(ax, ay, dx, dy, wx, wy), t = proj_t(ax, ay, dx, dy, wx, wy);
    e.smin = s < e.smin ? s : e.smin;
    e.smax = s > e.smax ? s : e.smax;
    e.tmax = t > e.tmax ? t : e.tmax;
}

struct Edge {
    double A, L2, smin, smax, tmax;
    int i;  // NO_EDGE: none
};
GPK_MB_FN Edge no_edge() { return Edge{INFINITY, 1.0, 0.0, 0.0, 0.0, NO_EDGE}; }
GPK_MB_FN Edge edge_of(int i, double dx, double dy, const Extent& e) {
    return Edge{(e.smax - e.smin) * e.tmax, dx * dx + dy * dy, e.smin, e.smax, e.tmax, i};
}
// is x the better edge: strictly less area, the lower index among equal areas
GPK_MB_FN bool edge_better(const Edge& x, const Edge& y) {
    if (x.i == NO_EDGE) return false;
    if (y.i == NO_EDGE) return true;
    const double l = x.A * y.L2, r = y.A * x.L2;
    return l < r || (l == r && x.i < y.i);
}
// the better of two (the same value whichever way round they are given, NaN areas included: reductions pair lanes symmetrically)
GPK_MB_FN Edge edge_pick(const Edge& x, const Edge& y) {
    const bool take_y = edge_better(y, x) || (!edge_better(x, y) && y.i < x.i);  // (field by field: the edges stay in registers)
    return Edge{take_y ? y.A : x.A, take_y ? y.L2 : x.L2, take_y ? y.smin : x.smin, take_y ? y.smax : x.smax, take_y ? y.tmax : x.tmax, take_y ? y.i : x.i};
}
// ---- rotating calipers (hulls too large for the quadratic scan) -------------------------------------------------------------------------
// The three support vertices of an edge — largest s, largest t, least s — each move on counter-clockwise from edge to edge.  Whether a
// support moves on is decided from the HULL EDGE e = v[k+1] - v[k] itself, never from two rounded projections: e . d > 0 (largest s),
// d x e > 0 (largest t), e . d <= 0 (least s).  Two projections of vertices an ulp apart round to the same value and would stall the
// advance long before the extreme; the difference of neighbouring vertices keeps its sign, and a sign can only come out wrong where the
// edge is within rounding of perpendicular (parallel for t) to d, which is at the extreme itself.  Relative to d the directions of the
// hull's edges turn monotonically, so from the support of one edge to that of the next every edge passed has the sign that moves on,
// whatever the turn between the two edges (below 180 degrees on a hull).  The extents are then the rule's own s and t of those vertices.
struct Calipers {
    int jmax, jtop, jmin;
};
// ld(k): vertex k as a struct with members x, y.  first: the supports start from the edge's own end vertex (a walk of at most h steps
// each); otherwise c holds the supports of the previous edge.  Every loop is bounded by h.
template <class LD>
GPK_MB_FN Edge caliper_edge(LD ld, int h, int i, bool first, Calipers& c) {
    const auto p = ld(i), q = ld(i + 1 == h ? 0 : i + 1);
    const double dx = q.x - p.x, dy = q.y - p.y;
    if (first) c.jmax = c.jtop = i + 1 == h ? 0 : i + 1;
    for (int st = 0; st < h; ++st) {
        const int k = c.jmax + 1 == h ? 0 : c.jmax + 1;
        const auto a = ld(c.jmax), b = ld(k);
        if (!((b.x - a.x) * dx + (b.y - a.y) * dy > 0.0)) break;
        c.jmax = k;
    }
    for (int st = 0; st < h; ++st) {
        const int k = c.jtop + 1 == h ? 0 : c.jtop + 1;
        const auto a = ld(c.jtop), b = ld(k);
        if (!(dx * (b.y - a.y) - dy * (b.x - a.x) > 0.0)) break;
        c.jtop = k;
    }
    if (first) c.jmin = c.jtop;  // (from the top vertex to the one of least s every edge runs against d)
    for (int st = 0; st < h; ++st) {
        const int k = c.jmin + 1 == h ? 0 : c.jmin + 1;
        const auto a = ld(c.jmin), b = ld(k);
        if (!((b.x - a.x) * dx + (b.y - a.y) * dy <= 0.0)) break;
        c.jmin = k;
    }
    const auto wmax = ld(c.jmax), wtop = ld(c.jtop), wmin = ld(c.jmin);
    Extent e = extent_start();  // (the rule's extremes start from a itself: s = t = 0)
    const double smax = proj_s(p.x, p.y, dx, dy, wmax.x, wmax.y), tmax = proj_t(p.x, p.y, dx, dy, wtop.x, wtop.y);
    const double smin = proj_s(p.x, p.y, dx, dy, wmin.x, wmin.y);
    e.smax = smax > e.smax ? smax : e.smax;
    e.tmax = tmax > e.tmax ? tmax : e.tmax;
    e.smin = smin < e.smin ? smin : e.smin;
    return edge_of(i, dx, dy, e);
}

// the corners c0 c1 c2 c3 of a rectangle (the ring is c0 c1 c2 c3 c0)
struct Rect {
    double x0, y0, x1, y1, x2, y2, x3, y3;
};
// the rectangle on edge e (a, d)
GPK_MB_FN Rect rect_corners(double ax, double ay, double dx, double dy, const Edge& e) {
    const double lo = e.smin / e.L2, hi = e.smax / e.L2, up = e.tmax / e.L2;
    const double nx = -dy, ny = dx;
    const double c0x = ax + lo * dx, c0y = ay + lo * dy;
    const double c1x = ax + hi * dx, c1y = ay + hi * dy;
    return Rect{c0x, c0y, c1x, c1y, c1x + up * nx, c1y + up * ny, c0x + up * nx, c0y + up * ny};
}
// the degenerate rows: one distinct point p (q = p), or the collinear hull ring p q p
GPK_MB_FN Rect rect_flat(double px, double py, double qx, double qy) { return Rect{px, py, qx, qy, qx, qy, px, py}; }

// ---- circle -------------------------------------------------------------------------------------------------------------------------
GPK_MB_FN double dist2(double px, double py, double cx, double cy) {
    const double dx = px - cx, dy = py - cy;
    return dx * dx + dy * dy;
}
// the farthest vertex so far: a later one only when strictly farther
struct Far {
    double d2;
    int index;  // NO_EDGE: none
};
GPK_MB_FN Far no_far() { return Far{-1.0, NO_EDGE}; }
GPK_MB_FN void far_see(Far& f, double d2, int index) {
    if (d2 > f.d2 || (d2 == f.d2 && index < f.index)) f = Far{d2, index};
}

struct Circle {
    double cx, cy, r2;    // row-local
    double sx[3], sy[3];  // support, row-local; [0] is the point the radius is measured to
    int si[3];            // hull indices of the support
    int ns;               // 2 or 3
};
struct Centre {
    double x, y;
    bool ok;
};
GPK_MB_FN Centre centre2(double ax, double ay, double bx, double by) { return Centre{(ax + bx) / 2, (ay + by) / 2, true}; }
GPK_MB_FN Centre centre3(double ax, double ay, double bx, double by, double cx, double cy) {
    const double ex = bx - ax, ey = by - ay, fx = cx - ax, fy = cy - ay;
    const double D = 2 * (ex * fy - ey * fx);
    const double e2 = ex * ex + ey * ey, f2 = fx * fx + fy * fy;
    if (!(D != 0.0)) return Centre{0.0, 0.0, false};
    return Centre{ax + (fy * e2 - ey * f2) / D, ay + (ex * f2 - fx * e2) / D, true};
}
// the circle on v_0 (the local origin, hull index 0) and the vertex (px, py) of hull index i
GPK_MB_FN Circle circle_start(double px, double py, int i) {
    Circle c;
    const Centre m = centre2(px, py, 0.0, 0.0);
    c.cx = m.x, c.cy = m.y;
    c.sx[0] = px, c.sy[0] = py, c.si[0] = i;
    c.sx[1] = 0.0, c.sy[1] = 0.0, c.si[1] = 0;
    c.sx[2] = 0.0, c.sy[2] = 0.0, c.si[2] = 0;
    c.ns = 2;
    c.r2 = dist2(px, py, c.cx, c.cy);
    return c;
}
GPK_MB_FN bool circle_has(const Circle& c, int index) {
    return c.si[0] == index || c.si[1] == index || (c.ns == 3 && c.si[2] == index);
}
// is the farthest vertex no reason to go on
GPK_MB_FN bool circle_done(const Circle& c, const Far& f) { return !(f.d2 > c.r2) || circle_has(c, f.index); }
// the O(1) step: the circle of least reach through q = (qx, qy) (hull index qi) and one or two of the old support points
// one candidate: q with the old support point I0 (I1 < 0), or with the pair I0, I1 (constant indices: the support stays in registers)
template <int I0, int I1>
GPK_MB_FN void circle_try(Circle& best, double& reach, const Circle& o, double qx, double qy, int qi) {
    if (I0 >= o.ns || I1 >= o.ns) return;
    const Centre m = I1 < 0 ? centre2(qx, qy, o.sx[I0], o.sy[I0]) : centre3(qx, qy, o.sx[I0], o.sy[I0], o.sx[I1 < 0 ? 0 : I1], o.sy[I1 < 0 ? 0 : I1]);
    if (!m.ok) return;
    const double rq = dist2(qx, qy, m.x, m.y);
    double e = rq;
    const double d0 = dist2(o.sx[0], o.sy[0], m.x, m.y), d1 = dist2(o.sx[1], o.sy[1], m.x, m.y), d2 = dist2(o.sx[2], o.sy[2], m.x, m.y);
    e = d0 > e ? d0 : e;
    e = d1 > e ? d1 : e;
    e = (o.ns == 3 && d2 > e) ? d2 : e;
    if (e < reach) {
        reach = e;
        best.cx = m.x, best.cy = m.y, best.r2 = rq;
        best.sx[0] = qx, best.sy[0] = qy, best.si[0] = qi;
        best.sx[1] = o.sx[I0], best.sy[1] = o.sy[I0], best.si[1] = o.si[I0];
        best.sx[2] = o.sx[I1 < 0 ? 0 : I1], best.sy[2] = o.sy[I1 < 0 ? 0 : I1], best.si[2] = o.si[I1 < 0 ? 0 : I1];
        best.ns = I1 < 0 ? 2 : 3;
    }
}
GPK_MB_FN Circle circle_step(const Circle& o, double qx, double qy, int qi) {
    Circle best = o;
    double reach = INFINITY;
    circle_try<0, -1>(best, reach, o, qx, qy, qi);
    circle_try<1, -1>(best, reach, o, qx, qy, qi);
    circle_try<2, -1>(best, reach, o, qx, qy, qi);
    circle_try<0, 1>(best, reach, o, qx, qy, qi);
    circle_try<0, 2>(best, reach, o, qx, qy, qi);
    circle_try<1, 2>(best, reach, o, qx, qy, qi);
    return best;
}

}  // namespace mb
}  // namespace gpk
