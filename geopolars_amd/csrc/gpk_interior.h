// gpk_interior.h — a point that stands for a row and lies in it: the per-edge and per-member rules of gpk_representative_point
// (include/geopolars_hip.h states the contract; DESIGN.md section 4.3l the schedules).  They follow GEOS's InteriorPointArea /
// InteriorPointLine / InteriorPointPoint.
//
// Polygonal rows, member by member (a member without rings or with an empty shell is ignored):
//   scan line   centreY = (miny + maxy) / 2 of the member's coordinates; loY = the largest ordinate <= centreY, hiY = the smallest
//               ordinate > centreY (miny / maxy when there is none); scanY = (loY + hiY) / 2.  Comparisons and one average: the same
//               bits on every machine.  The line passes between two vertex ordinates, so it meets edges inside them — unless loY and
//               hiY are adjacent doubles, when the average is one of them.
//   crossings   every non-horizontal edge whose closed y-range holds scanY, but for an edge that meets the line at its UPPER end only
//               (edge_counts): a vertex on the line then counts once for a boundary that passes through it and twice or not at all
//               for one that turns back.  x = x0 for a vertical edge, else x0 + (scanY - y0) * ((x1 - x0) / (y1 - y0)), in exactly
//               this order of operations and without contraction.
//   sections    the crossings in ascending order of (x, edge index) pair up: (0, 1), (2, 3), ...; width = x[2k + 1] - x[2k].
//   choice      the widest section, the lowest rank among equal widths; over the members a later one only when strictly wider.  The
//               point is ((x[2k] + x[2k + 1]) / 2, scanY).  No section of positive width: the row's first coordinate, width 0.
// Lineal rows: the interior vertex (neither first nor last of its member) nearest to the row's centroid, the nearest member end point
// when the row has no interior vertex.  Puntal rows: the member nearest to the mean.  Distance dx * dx + dy * dy, a later candidate only
// when strictly nearer.
//
// Everything in this file is plain C++ (no HIP type, no intrinsic): the device kernels (gpk_interior.hip) and a host program
// (tests/interior_host_driver.cpp) run the same functions.
//
// Schedules (gpk_interior.hip).  G lanes per row (G = 4 or 16 from the column's mean coordinate count) for rows of at most
// INT_BLOCK_COORDS coordinates; the crossings of a member go to a slice of INT_SLICE entries of LDS that the group owns, every entry is
// ranked against all of them (k^2 / G comparisons for k crossings).  A member with more crossings than the slice holds puts the row on
// the list of the work-group kernel, which also takes the rows above INT_BLOCK_COORDS: crossings appended to an LDS list of
// INT_LDS_CROSSINGS entries (one LDS atomic each), bitonic sort on (x, edge index), reduction over the even positions.
// A member with more crossings than that list holds is NOT spilled to global memory: a scratch buffer would have to be sized by the
// column's coordinate count (12 bytes a coordinate, 1.5 GB for 2M rows of 64) for a case that needs a ring of thousands of zigzags.
// Instead the work-group ranks without a list: every thread takes edges strided, and for each of its counted edges walks all edges of
// the member again, recomputing their crossings (crossing_x is a pure function: the same bits), to find the rank and the successor.
// Cost: k * n / INT_BLOCK_THREADS crossing evaluations per thread for k crossings among n edges — 4 x 10^6 for a ring of 10^5
// coordinates crossed 10^4 times — and no memory at all.  The bound is quadratic: a sawtooth ring of 10^6 coordinates that the line
// crosses 5 x 10^5 times costs its one work-group 2 x 10^9 evaluations per thread, minutes of one compute unit.  A list in global memory,
// (largest row) x (work-groups launched) entries after a pass that finds the largest row, with a sort in passes, would bring that to
// k log^2 k / INT_BLOCK_THREADS; it is not built.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define GPK_IP_FN __host__ __device__ __forceinline__
#else
#define GPK_IP_FN inline
#endif

namespace gpk {
namespace ip {

constexpr int INT_G_SMALL = 4, INT_G_LARGE = 16;
constexpr double INT_G_MEAN = 32.0;        // columns of at least this many coordinates a row on average take INT_G_LARGE
constexpr int INT_BLOCK_COORDS = 512;      // rows of more coordinates take the work-group path
constexpr int INT_BLOCK_THREADS = 256;
constexpr int INT_SLICE = 32;              // crossings of one member a lane group keeps in LDS
constexpr int INT_LDS_CROSSINGS = 2048;    // crossings of one member the work-group sorts in LDS (a power of two)
constexpr int NO_RANK = 0x7fffffff;

// ---- the scan line ------------------------------------------------------------------------------------------------------------------
GPK_IP_FN double centre_y(double miny, double maxy) { return (miny + maxy) / 2; }
// one ordinate of the member: lo and hi start at miny and maxy
GPK_IP_FN void scan_update(double y, double centre, double& lo, double& hi) {
    lo = (y <= centre && y > lo) ? y : lo;  // (two selects, not a branch that picks which of the two to store to)
    hi = (y > centre && y < hi) ? y : hi;
}
GPK_IP_FN double scan_y(double lo, double hi) { return (lo + hi) / 2; }

// ---- crossings ----------------------------------------------------------------------------------------------------------------------
// does the edge (y0 -> y1) give a crossing of the line y = scan
GPK_IP_FN bool edge_counts(double y0, double y1, double scan) {
    if (y0 == y1) return false;
    if ((y0 > scan && y1 > scan) || (y0 < scan && y1 < scan)) return false;
    if (y0 == scan && y1 < scan) return false;  // the line meets the edge at its upper end only
    if (y1 == scan && y0 < scan) return false;
    return true;
}
GPK_IP_FN double crossing_x(double x0, double y0, double x1, double y1, double scan) {
    if (x0 == x1) return x0;
    const double slope = (x1 - x0) / (y1 - y0);
    const double run = (scan - y0) * slope;
    return x0 + run;
}
// the order of the crossings: by x, equal x by edge index
GPK_IP_FN bool crossing_less(double xa, int ea, double xb, int eb) { return xa < xb || (xa == xb && ea < eb); }

// ---- sections -----------------------------------------------------------------------------------------------------------------------
// What one crossing (x, e) learns from walking over the others: its rank (how many are less) and its successor (the least of the
// greater ones).  An even-ranked crossing with a successor opens the section (x, succ_x).
struct Ranked {
    int rank;
    bool has_succ;
    double succ_x;
    int succ_e;
};
GPK_IP_FN Ranked ranked_start() { return Ranked{0, false, 0.0, 0}; }
GPK_IP_FN void ranked_see(Ranked& r, double x, int e, double ox, int oe) {
    if (crossing_less(ox, oe, x, e)) {
        ++r.rank;
    } else if (crossing_less(x, e, ox, oe)) {
        if (!r.has_succ || crossing_less(ox, oe, r.succ_x, r.succ_e)) {
            r.has_succ = true;
            r.succ_x = ox;
            r.succ_e = oe;
        }
    }
}

// the best section so far of a member (by width, equal widths by rank) or of a row (members fold with the strict rule)
struct Section {
    double width, x;
    int rank;  // NO_RANK: none
};
GPK_IP_FN Section no_section() { return Section{0.0, 0.0, NO_RANK}; }
GPK_IP_FN bool section_better(double w, int rank, const Section& s) { return w > s.width || (w == s.width && rank < s.rank); }
// the section that opens at the crossing x of even rank `rank` and closes at x1
GPK_IP_FN void section_propose(Section& s, double x, double x1, int rank) {
    const double w = x1 - x;
    if (w > 0.0 && section_better(w, rank, s)) s = Section{w, (x + x1) / 2, rank};
}

struct RowPoint {
    double width, x, y;
};
// the member's best section against the row's: a later member only when strictly wider
GPK_IP_FN void member_fold(RowPoint& row, const Section& s, double scan) {
    if (s.rank != NO_RANK && s.width > row.width) row = RowPoint{s.width, s.x, scan};
}

// ---- nearest vertex -------------------------------------------------------------------------------------------------------------------
GPK_IP_FN double dist2(double px, double py, double cx, double cy) {
    const double dx = px - cx, dy = py - cy;
    return dx * dx + dy * dy;
}
struct Nearest {
    double d;
    int index;  // NO_RANK: none
};
GPK_IP_FN Nearest no_nearest() { return Nearest{INFINITY, NO_RANK}; }
GPK_IP_FN void nearest_see(Nearest& n, double d, int index) {
    if (d < n.d || (d == n.d && index < n.index)) n = Nearest{d, index};
}

}  // namespace ip
}  // namespace gpk
