// gpk_nearwalk.h — the seed walk of gpk_nearest_join_any (gpk_nearest_any.hip): for one left BOX, the right row whose box is nearest to
// it, found in the right side's bbox grid directory without reading a coordinate.  The rule is the walk of nearest_walk
// (gpk_nearest.hip) with box-to-box distances in place of point-to-box distances; it compiles for the host as well, where
// tests/nearwalk_host_driver.cpp runs it against a brute-force minimum.
//
// The walk.  The visited rectangle of cells starts as the cells the left box covers, each corner clamped onto the grid (a box outside
// the extent starts in border cells and never walks the empty gap; a box covering the extent starts with every cell).  It then grows
// one column or row at a time on the side whose unvisited part — a rectangle of the extent: every cell beyond that side — is nearest
// to the left box, and stops once the nearest unvisited part is farther than the bound: the distance of the nearest box found so far,
// `max_d` before one is found.  Strictly farther, so a box exactly as far as the best one is still reached and the LOWEST row id among
// the nearest boxes wins.  A cell farther than the bound is skipped without reading its entries.
//
// Why the nearest box is found.  A right row is listed in every cell its closed box meets, under the monotone cell function the
// directory was built with (cell_of below restates dev::cell_of).  The point of the right box nearest to the left box lies in one of
// those cells, and that cell's rectangle is no farther from the left box than the right box is; so is every part of the extent that
// holds the cell.  The walk passes over a cell or a part only when it is farther than the bound, hence farther than that row's box.
// Cell borders come from the rounded cell function and the distances from rounded arithmetic: every comparison with the bound gives
// way by m = 64 eps (|x0| + |y0| + extent width + extent height + the left box's |coordinates|), the convention of gpk_nearest.hip.
// A row with two or more boxes in its list is met more than once: taking a minimum does not mind.
//
// Bounds.  The start rectangle has at most ex * ey cells, the growth at most ex + ey steps of at most max(ex, ey) cells: every loop is
// bounded by the grid's dimensions and the directory's lists.  An axis of zero extent (inv == 0: the cell function sends everything
// to column / row 0) has one usable column / row of width 0.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GPK_NW_FN __host__ __device__ __forceinline__
#else
#define GPK_NW_FN inline
#endif

namespace gpk {
namespace nw {

constexpr uint32_t NO_SEED = 0xFFFFFFFFu;

struct Grid {
    double x0, y0, inv_w, inv_h;  // the directory's own parameters (the cell function)
    double cw, ch;                // cell width / height (0 on a degenerate axis)
    double scale;                 // |x0| + |y0| + extent width + extent height: the magnitude the margins scale with
    int32_t gx, gy;               // directory dimensions (cell id = cy * gx + cx)
    int32_t ex, ey;               // usable columns / rows
};
struct Box {
    double x0, y0, x1, y1;
};

GPK_NW_FN Grid make_grid(double x0, double y0, double inv_w, double inv_h, int32_t gx, int32_t gy) {
    Grid g;
    g.x0 = x0;
    g.y0 = y0;
    g.inv_w = inv_w;
    g.inv_h = inv_h;
    g.gx = gx;
    g.gy = gy;
    g.cw = inv_w > 0.0 ? 1.0 / inv_w : 0.0;
    g.ch = inv_h > 0.0 ? 1.0 / inv_h : 0.0;
    g.ex = inv_w > 0.0 ? gx : 1;
    g.ey = inv_h > 0.0 ? gy : 1;
    g.scale = fabs(x0) + fabs(y0) + g.ex * g.cw + g.ey * g.ch;
    return g;
}

// dev::cell_of (gpk_index.h): negative / NaN products clamp to 0, large ones to g - 1; truncation is floor() on the clamped value
GPK_NW_FN int cell_of(double v, double v0, double inv, int g) { return (int)fmin(fmax((v - v0) * inv, 0.0), (double)(g - 1)); }

// (fmax drops a NaN: a box with a NaN must be refused BEFORE this is asked)
GPK_NW_FN bool box_ok(const Box& b) { return b.x0 <= b.x1 && b.y0 <= b.y1; }
GPK_NW_FN double box_distance(const Box& a, const Box& b) {
    const double dx = fmax(fmax(b.x0 - a.x1, a.x0 - b.x1), 0.0), dy = fmax(fmax(b.y0 - a.y1, a.y0 - b.y1), 0.0);
    return sqrt(dx * dx + dy * dy);
}
GPK_NW_FN double margin(const Grid& g, const Box& L) { return 64.0 * DBL_EPSILON * (g.scale + fabs(L.x0) + fabs(L.y0) + fabs(L.x1) + fabs(L.y1)); }

// Dir: int cell_begin(int c), int cell_end(int c) (the cell's slice of the item list), uint32_t item(int k), bool usable(uint32_t j)
// (the right row is valid), Box box(uint32_t j).
// Returns the lowest row among those whose box is nearest to L — the box distance goes to *seed_bd — or NO_SEED when L holds a NaN or
// no usable box lies within max_d + m.
template <class Dir>
GPK_NW_FN uint32_t seed_walk(const Grid& g, const Dir& dir, const Box& L, double max_d, double* seed_bd) {
    *seed_bd = INFINITY;
    if (!box_ok(L)) return NO_SEED;
    const double m = margin(g, L);
    double best = INFINITY;
    uint32_t seed = NO_SEED;
    auto visit = [&](int cx, int cy) {
        const double ax = g.x0 + cx * g.cw, ay = g.y0 + cy * g.ch;
        const double bound = best < max_d ? best : max_d;
        if (box_distance(L, Box{ax, ay, ax + g.cw, ay + g.ch}) - m > bound) return;
        const int c = cy * g.gx + cx;
        const int k1 = dir.cell_end(c);
        for (int k = dir.cell_begin(c); k < k1; ++k) {
            const uint32_t j = dir.item(k);
            if (!dir.usable(j)) continue;
            const Box b = dir.box(j);
            if (!box_ok(b)) continue;
            const double bd = box_distance(L, b);
            if (!(bd - m <= max_d)) continue;
            if (bd < best || (bd == best && j < seed)) {
                best = bd;
                seed = j;
            }
        }
    };
    int ax0 = cell_of(L.x0, g.x0, g.inv_w, g.gx), ax1 = cell_of(L.x1, g.x0, g.inv_w, g.gx);
    int ay0 = cell_of(L.y0, g.y0, g.inv_h, g.gy), ay1 = cell_of(L.y1, g.y0, g.inv_h, g.gy);
    if (ax0 >= g.ex) ax0 = g.ex - 1;
    if (ax1 >= g.ex) ax1 = g.ex - 1;
    if (ay0 >= g.ey) ay0 = g.ey - 1;
    if (ay1 >= g.ey) ay1 = g.ey - 1;
    for (int cy = ay0; cy <= ay1; ++cy)
        for (int cx = ax0; cx <= ax1; ++cx) visit(cx, cy);
    const double X0 = g.x0, X1 = g.x0 + g.ex * g.cw, Y0 = g.y0, Y1 = g.y0 + g.ey * g.ch;
    for (int step = 0; step < g.ex + g.ey; ++step) {
        // distance to the unvisited cells beyond each side of the visited rectangle (all rows / columns of the extent)
        const double dl = ax0 > 0 ? box_distance(L, Box{X0, Y0, g.x0 + ax0 * g.cw, Y1}) : INFINITY;
        const double dr = ax1 < g.ex - 1 ? box_distance(L, Box{g.x0 + (ax1 + 1) * g.cw, Y0, X1, Y1}) : INFINITY;
        const double db = ay0 > 0 ? box_distance(L, Box{X0, Y0, X1, g.y0 + ay0 * g.ch}) : INFINITY;
        const double dt = ay1 < g.ey - 1 ? box_distance(L, Box{X0, g.y0 + (ay1 + 1) * g.ch, X1, Y1}) : INFINITY;
        int side = 0;
        double lo = dl;
        if (dr < lo) lo = dr, side = 1;
        if (db < lo) lo = db, side = 2;
        if (dt < lo) lo = dt, side = 3;
        const double bound = best < max_d ? best : max_d;
        if (lo == INFINITY || lo - m > bound) break;
        if (side < 2) {  // a new column, bottom to top
            const int cx = side == 0 ? --ax0 : ++ax1;
            for (int cy = ay0; cy <= ay1; ++cy) visit(cx, cy);
        } else {  // a new row, left to right
            const int cy = side == 2 ? --ay0 : ++ay1;
            for (int cx = ax0; cx <= ax1; ++cx) visit(cx, cy);
        }
    }
    *seed_bd = best;
    return seed;
}

}  // namespace nw
}  // namespace gpk
