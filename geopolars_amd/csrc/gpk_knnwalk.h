// gpk_knnwalk.h — the k-seed walk of gpk_knn_join (gpk_knn.hip): for one left BOX, the K usable right rows whose boxes have the smallest
// FAR distance to it, found in the right side's bbox grid directory without reading a coordinate.  Grid, Box, Dir, the cell function and
// the margin are those of gpk_nearwalk.h; like it the walk compiles for the host, where tests/knnwalk_host_driver.cpp runs it against
// brute force.
//
// Why far distances.  The far distance of two boxes — the largest distance between a point of one and a point of the other — bounds the
// exact distance of the two rows from above, whatever their shapes: K distinct usable rows with far distance <= F lie within F of the
// left row, so the k-th neighbour does too.  That gives gpk_knn_join its search radius from the directory alone; the alternative, the K
// nearest boxes and their exact distances, costs K exact evaluations per left row before the first candidate is listed.  For POINT x
// POINT the far distance IS the distance and the radius is the k-th neighbour's own.
//
// The rule.  A key is (far distance, right row), compared lexicographically: ties go to the lower row.  The result is the K lowest keys
// among the usable right rows with far distance <= max_d, ascending, each row once; fewer when fewer exist.
//
// The walk.  The visited rectangle of cells starts and grows as in gpk_nearwalk.h, by the NEAR distance of the unvisited parts of the
// extent.  It stops once the nearest unvisited part is strictly farther than the bound plus margin; the bound is the K-th lowest far
// distance so far, max_d while fewer than K rows are held.  A cell farther than the bound is skipped without reading its entries.
//
// Why the K lowest keys are found.  A right row is listed in every cell its closed box meets, and the cell that holds the point of the
// box nearest to the left box is no farther from the left box than the row's near distance, nor is any part of the extent holding that
// cell (the argument of gpk_nearwalk.h, margin included).  The near distance of a box is at most its far distance — also as computed:
// each term of the near distance is a difference that is no larger than the far distance's term, and rounding, fmax and sqrt are
// monotone.  So a row the walk passed over has near distance > bound, hence far distance > bound: it is not among the K lowest, or not
// within max_d.
//
// One slot per row.  A row that spans cells is met once per cell.  Its key is the same every time, and the list is sorted: the
// insertion finds the position of the key and drops it when the entry there is the same row.  A row that was pushed out of a full list
// has a key above the list's last and is refused before that.
//
// Bounds.  The loops of gpk_nearwalk.h, with at most K entries moved per inserted row.
#pragma once

#include "gpk_nearwalk.h"

namespace gpk {
namespace nw {

GPK_NW_FN double box_far_distance(const Box& a, const Box& b) {
    const double dx = fmax(b.x1 - a.x0, a.x1 - b.x0), dy = fmax(b.y1 - a.y0, a.y1 - b.y0);
    return sqrt(dx * dx + dy * dy);
}

// Slots: double& far(int s), uint32_t& row(int s) for s in [0, K) — the caller's storage (LDS on the device).
// Returns the number of slots filled, sorted ascending by (far, row); 0 when L holds a NaN.
template <class Dir, class Slots>
GPK_NW_FN int knn_seed_walk(const Grid& g, const Dir& dir, const Box& L, double max_d, int K, Slots& slots) {
    if (!box_ok(L)) return 0;
    const double m = margin(g, L);
    int held = 0;
    auto bound_now = [&]() {
        const double kth = held == K ? slots.far(K - 1) : INFINITY;
        return kth < max_d ? kth : max_d;
    };
    auto visit = [&](int cx, int cy) {
        const double ax = g.x0 + cx * g.cw, ay = g.y0 + cy * g.ch;
        if (box_distance(L, Box{ax, ay, ax + g.cw, ay + g.ch}) - m > bound_now()) return;
        const int c = cy * g.gx + cx;
        const int k1 = dir.cell_end(c);
        for (int k = dir.cell_begin(c); k < k1; ++k) {
            const uint32_t j = dir.item(k);
            if (!dir.usable(j)) continue;
            const Box b = dir.box(j);
            if (!box_ok(b)) continue;
            const double fd = box_far_distance(L, b);
            if (!(fd <= max_d)) continue;
            if (held == K && !(fd < slots.far(K - 1) || (fd == slots.far(K - 1) && j < slots.row(K - 1)))) continue;
            int p = 0;  // the first entry whose key is not below (fd, j)
            while (p < held && (slots.far(p) < fd || (slots.far(p) == fd && slots.row(p) < j))) ++p;
            if (p < held && slots.row(p) == j && slots.far(p) == fd) continue;  // the same row from another cell
            const int last = held < K ? held : K - 1;
            for (int s = last; s > p; --s) slots.far(s) = slots.far(s - 1), slots.row(s) = slots.row(s - 1);
            slots.far(p) = fd;
            slots.row(p) = j;
            if (held < K) ++held;
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
        const double dl = ax0 > 0 ? box_distance(L, Box{X0, Y0, g.x0 + ax0 * g.cw, Y1}) : INFINITY;
        const double dr = ax1 < g.ex - 1 ? box_distance(L, Box{g.x0 + (ax1 + 1) * g.cw, Y0, X1, Y1}) : INFINITY;
        const double db = ay0 > 0 ? box_distance(L, Box{X0, Y0, X1, g.y0 + ay0 * g.ch}) : INFINITY;
        const double dt = ay1 < g.ey - 1 ? box_distance(L, Box{X0, g.y0 + (ay1 + 1) * g.ch, X1, Y1}) : INFINITY;
        int side = 0;
        double lo = dl;
        if (dr < lo) lo = dr, side = 1;
        if (db < lo) lo = db, side = 2;
        if (dt < lo) lo = dt, side = 3;
        if (lo == INFINITY || lo - m > bound_now()) break;
        if (side < 2) {
            const int cx = side == 0 ? --ax0 : ++ax1;
            for (int cy = ay0; cy <= ay1; ++cy) visit(cx, cy);
        } else {
            const int cy = side == 2 ? --ay0 : ++ay1;
            for (int cx = ax0; cx <= ax1; ++cx) visit(cx, cy);
        }
    }
    return held;
}

}  // namespace nw
}  // namespace gpk
