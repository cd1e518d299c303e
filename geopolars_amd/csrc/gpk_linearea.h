// gpk_linearea.h — where a line runs relative to a polygonal geometry: the 3-bit mask of gpk_line_polygon_relation
// (include/geopolars_hip.h).  L = a LINESTRING / MULTILINESTRING row, the closed set of its segments and coordinates; P = a POLYGON /
// MULTIPOLYGON row.  GPK_LP_INTERIOR: L has a point in P's interior, GPK_LP_BOUNDARY: on a ring of P, GPK_LP_EXTERIOR: outside every
// part or strictly inside a hole.  Interior and exterior are open, so every named line / area predicate is a function of the mask.
//
//   mask = OR over the coordinates c of L of position(c, P)
//        | OR over the events (t, w) of side(t -> w, P)
// An event is a touch of a segment pq of L (p != q) with a ring, taken with a direction w (p or q):
//   1. p or q lies on a ring (its position is BOUNDARY): (p, q) or (q, p);
//   2. a ring vertex a lies on the open segment: (a, p) and (a, q);
//   3. pq crosses a ring edge ab properly (inside both): the crossed ring has one side on either hand and, unless another ring has a
//      vertex at the crossing point, is the only ring there — the mask is complete (7).  A vertex v of P at the crossing point (v in
//      the segment's box, orient(p, q, v) == 0, orient(a, b, v) == 0 — exact, though the point itself may not be representable) is an
//      event of kind 2 of the same segment, which judges both directions against the whole geometry: the crossing then adds nothing.
// Between two consecutive touch points a segment stays in P's interior or exterior or on one ring edge, and the piece next to a touch
// point is judged there, so every piece of L is seen.  side(t -> w, P): the piece of the segment t -> w next to t against EVERY ring of
// every part — rings of a valid geometry may touch each other at single points (hole-shell, hole-hole, part-part), and a line may pass
// through such a point, so the ring that was hit does not decide alone.  Against a ring that does not hold t the piece lies where t
// lies; at a vertex of the ring the sector test cont::dir_at_vertex decides, inside an edge the edge's side; a piece that runs along
// an edge is BOUNDARY.  Inside a part = inside its shell and outside its holes; INTERIOR if inside some part, else EXTERIOR.
// Every sign is an exact orientation (gpk_device.h): no tolerance, the same mask at any placement of the same figure.
//
// G lanes work on one (L, P) pair: ring edges are strided over the lanes, the coordinate, segment or event under test is the same on
// all of them, verdicts are group-wide ORs (every branch around a reduction is group-uniform, as the DPP reductions need).
// Cost: segments x edges orientation tests per pair (box-pruned), coordinates x edges for the positions, plus one pass over the whole
// geometry per event and direction.  A segment whose box misses the box of P's shells is skipped, a coordinate outside it is EXTERIOR.
//
// Rows: a null line, one without a coordinate or with a NaN coordinate: 0.  A null polygon or one without a non-empty member: 0.  A
// non-empty ring that fails cont::ring_init (unclosed, fewer than 4 coordinates, NaN, no turning extreme vertex): 0 — the rule and the
// decision of `contains`.  Empty members are ignored.  A one-coordinate sequence and repeated coordinates are the point set of their
// coordinates.  Invalid polygons (self-crossing rings, overlapping parts): the mask is unspecified, the routine terminates.
#pragma once

#include "gpk_contains.h"
#include "gpk_device.h"
#include "gpk_pairdist.h"
#include "gpk_polypoly.h"

namespace gpk {
namespace lp {

constexpr int LP_ALL = GPK_LP_INTERIOR | GPK_LP_BOUNDARY | GPK_LP_EXTERIOR;

// When a caller needs less than the mask: stop as soon as one of `any` is set or all of `all` are.  {0, LP_ALL}: the full mask.
struct Stop {
    int any, all;
};
__device__ __forceinline__ bool done(int mask, Stop st) { return (mask & st.any) != 0 || (mask & st.all) == st.all; }

// the predicate ids of gpk_line_polygon_join over the mask
__host__ __device__ inline bool predicate_of(int mask, int pred) {
    switch (pred) {
    case GPK_LP_PRED_INTERSECTS: return (mask & (GPK_LP_INTERIOR | GPK_LP_BOUNDARY)) != 0;
    case GPK_LP_PRED_WITHIN: return (mask & GPK_LP_INTERIOR) && !(mask & GPK_LP_EXTERIOR);
    case GPK_LP_PRED_COVERED_BY: return mask != 0 && !(mask & GPK_LP_EXTERIOR);
    case GPK_LP_PRED_CROSSES: return (mask & GPK_LP_INTERIOR) && (mask & GPK_LP_EXTERIOR);
    case GPK_LP_PRED_TOUCHES: return (mask & GPK_LP_BOUNDARY) && !(mask & GPK_LP_INTERIOR);
    default: return false;
    }
}
// the bits that settle a predicate before the mask is complete (covered_by stops at the first EXTERIOR bit, ...)
inline Stop stop_of(int pred) {
    switch (pred) {
    case GPK_LP_PRED_INTERSECTS: return Stop{GPK_LP_INTERIOR | GPK_LP_BOUNDARY, LP_ALL};
    case GPK_LP_PRED_WITHIN:
    case GPK_LP_PRED_COVERED_BY: return Stop{GPK_LP_EXTERIOR, LP_ALL};
    case GPK_LP_PRED_CROSSES: return Stop{0, GPK_LP_INTERIOR | GPK_LP_EXTERIOR};
    case GPK_LP_PRED_TOUCHES: return Stop{GPK_LP_INTERIOR, LP_ALL};
    default: return Stop{0, LP_ALL};
    }
}

template <int G>
__device__ __forceinline__ int group_imin(int v) {
    return dev::group_allreduce<G>(v, [](int a, int b) { return a < b ? a : b; });
}

// is part p of P a member with coordinates (an empty member adds nothing to the set), and its rings
__device__ __forceinline__ bool part_of(const DevGeo& P, int p, int& r0, int& r1) {
    dev::part_rings(P, p, r0, r1);
    return r1 > r0 && P.ring_off[r0 + 1] > P.ring_off[r0];
}

// The usable polygon row: every non-empty ring of every non-empty member passes ring_init, and there is such a member.  `box`: the
// box of the members' shells.
template <int G>
__device__ inline bool polygon_row_ok(const DevGeo& P, int p0, int p1, int lane, double4& box) {
    int members = 0;
    box = make_double4(INFINITY, INFINITY, -INFINITY, -INFINITY);
    for (int p = p0; p < p1; ++p) {
        int r0, r1;
        if (!part_of(P, p, r0, r1)) continue;
        if (!cont::rings_valid<G>(P, r0, r1, lane)) return false;
        const int c0 = P.ring_off[r0];
        const double4 b = cont::ring_bbox<G>(P.xy + c0, P.ring_off[r0 + 1] - c0, lane);
        box = make_double4(fmin(box.x, b.x), fmin(box.y, b.y), fmax(box.z, b.z), fmax(box.w, b.w));
        ++members;
    }
    return members > 0;
}

// position(c, P) as a mask bit.  On a ring of any member: BOUNDARY (the members of a valid geometry do not overlap, so a point on one
// member's ring is in no other member's interior).
template <int G>
__device__ inline int coord_bits(const DevGeo& P, int p0, int p1, double4 box, double2 c, int lane) {
    if (c.x < box.x || c.x > box.z || c.y < box.y || c.y > box.w) return GPK_LP_EXTERIOR;
    int in = 0;
    for (int p = p0; p < p1; ++p) {
        int r0, r1;
        dev::part_rings(P, p, r0, r1);
        const int pos = polygon_pos_group<G>(P, r0, r1, c.x, c.y, lane);  // (an empty member: outside)
        if (pos == dev::POS_BOUNDARY) return GPK_LP_BOUNDARY;
        in |= pos == dev::POS_INSIDE ? 1 : 0;
    }
    return in ? GPK_LP_INTERIOR : GPK_LP_EXTERIOR;
}

// The piece of the segment t -> w (t != w) next to t against one valid ring: cont::DIR_IN, cont::DIR_OUT, or 0 when it runs along the
// ring.  A ring that does not hold t has the piece where t is.
template <int G>
__device__ inline int ring_side(const double2* __restrict__ xy, int n, double2 t, double2 w, int lane) {
    const int pos = coord_pos_ring_group<G>(xy, n, t.x, t.y, lane);
    if (pos != dev::POS_BOUNDARY) return pos == dev::POS_INSIDE ? cont::DIR_IN : cont::DIR_OUT;
    cont::Ring r;
    (void)cont::ring_init<G>(r, xy, n, lane);
    // where on the ring: the lowest vertex equal to t, else the lowest edge with t strictly inside
    int vi = 0x7fffffff, ei = 0x7fffffff;
    for (int i = lane; i < r.m; i += G) {
        const double2 a = r.v[i], b = r.v[i + 1];
        if (cont::same_xy(a, t)) {
            vi = vi < i ? vi : i;
        } else if (ei == 0x7fffffff && !cont::same_xy(a, b) && cont::strictly_between(t, a, b) && cont::orient(a, b, t) == 0) {
            ei = i;
        }
    }
    vi = group_imin<G>(vi);
    if (vi != 0x7fffffff) return cont::dir_at_vertex(r, vi, w);
    ei = group_imin<G>(ei);
    if (ei == 0x7fffffff) return 0;  // (cannot happen: BOUNDARY means on a vertex or inside an edge)
    const int o = cont::orient(r.v[ei], r.v[ei + 1], w) * r.ccw;
    return o > 0 ? cont::DIR_IN : (o < 0 ? cont::DIR_OUT : 0);
}

// side(t -> w, P) as a mask bit: the piece next to t against every ring of every member
template <int G>
__device__ inline int side_bits(const DevGeo& P, int p0, int p1, double2 t, double2 w, int lane) {
    int in = 0;
    for (int p = p0; p < p1; ++p) {
        int r0, r1;
        if (!part_of(P, p, r0, r1)) continue;
        int c0 = P.ring_off[r0];
        const int s = ring_side<G>(P.xy + c0, P.ring_off[r0 + 1] - c0, t, w, lane);
        if (s == 0) return GPK_LP_BOUNDARY;
        if (s == cont::DIR_OUT) continue;
        bool inside = true;
        for (int r = r0 + 1; r < r1 && inside; ++r) {
            c0 = P.ring_off[r];
            const int n = P.ring_off[r + 1] - c0;
            if (n == 0) continue;
            const int h = ring_side<G>(P.xy + c0, n, t, w, lane);
            if (h == 0) return GPK_LP_BOUNDARY;
            inside = h == cont::DIR_OUT;
        }
        in |= inside ? 1 : 0;
    }
    return in ? GPK_LP_INTERIOR : GPK_LP_EXTERIOR;
}

// events of kinds 2 and 3 of segment pq on ring edge ab: bit 0 — a lies on the open segment; bit 1 — a proper crossing
__device__ __forceinline__ int edge_events(double2 p, double2 q, double lx, double hx, double ly, double hy, double2 a, double2 b) {
    if (fmax(a.x, b.x) < lx || fmin(a.x, b.x) > hx || fmax(a.y, b.y) < ly || fmin(a.y, b.y) > hy) return 0;
    const int oa = cont::orient(p, q, a);
    int e = 0;
    if (oa == 0 && a.x >= lx && a.x <= hx && a.y >= ly && a.y <= hy && !cont::same_xy(a, p) && !cont::same_xy(a, q)) e = 1;
    if (oa == 0 || cont::same_xy(a, b)) return e;
    if (oa * cont::orient(p, q, b) < 0 && cont::orient(a, b, p) * cont::orient(a, b, q) < 0) e |= 2;
    return e;
}

// does a vertex of P (coordinates [c0, c1) of the row) lie where pq crosses ab properly
template <int G>
__device__ inline bool vertex_at_crossing(const double2* __restrict__ xy, int c0, int c1, double2 p, double2 q, double lx, double hx, double ly,
                                          double hy, double2 a, double2 b, int lane) {
    int hit = 0;
    for (int i = c0 + lane; i < c1; i += G) {
        const double2 v = xy[i];
        if (v.x < lx || v.x > hx || v.y < ly || v.y > hy) continue;
        if (cont::orient(p, q, v) == 0 && cont::orient(a, b, v) == 0) hit = 1;
    }
    return dev::group_or<G>(hit) != 0;
}

// the mask bits of the events of kinds 2 and 3 of segment pq (p != q, its box meets the geometry's)
template <int G>
__device__ inline int segment_events(const DevGeo& P, int p0, int p1, double2 p, double2 q, int lane) {
    static_assert(G <= 16, "two event bits per lane in one word");
    const double lx = fmin(p.x, q.x), hx = fmax(p.x, q.x), ly = fmin(p.y, q.y), hy = fmax(p.y, q.y);
    const int32_t* part_ring = P.type == GPK_GEOM_MULTIPOLYGON ? P.part_off : P.geom_off;
    const int row_c0 = P.ring_off[part_ring[p0]], row_c1 = P.ring_off[part_ring[p1]];  // the row's coordinates are contiguous
    int bits = 0;
    for (int pt = p0; pt < p1; ++pt) {
        int r0, r1;
        if (!part_of(P, pt, r0, r1)) continue;
        for (int r = r0; r < r1; ++r) {
            const int c0 = P.ring_off[r], m = P.ring_off[r + 1] - c0 - 1;
            if (m < 1) continue;
            const double2* __restrict__ v = P.xy + c0;
            int ev = 0;
            for (int i = lane; i < m; i += G) ev |= edge_events(p, q, lx, hx, ly, hy, v[i], v[i + 1]);
            if (!dev::group_or<G>(ev)) continue;
            // a touched ring once more, a round of G edges at a time: the group takes the round's events one after the other
            bits |= GPK_LP_BOUNDARY;
            for (int base = 0; base < m; base += G) {
                const int i = base + lane;
                const int e = i < m ? edge_events(p, q, lx, hx, ly, hy, v[i], v[i + 1]) : 0;
                unsigned evs = (unsigned)dev::group_or<G>(e << (2 * lane));
                while (evs) {
                    const int k = (__ffs((int)evs) - 1) >> 1;
                    const int kind = (int)(evs >> (2 * k)) & 3;
                    evs &= ~(3u << (2 * k));
                    const double2 a = v[base + k], b = v[base + k + 1];
                    if (kind & 1) bits |= side_bits<G>(P, p0, p1, a, q, lane) | side_bits<G>(P, p0, p1, a, p, lane);
                    if ((kind & 2) && !vertex_at_crossing<G>(P.xy, row_c0, row_c1, p, q, lx, hx, ly, hy, a, b, lane)) return LP_ALL;
                    if (bits == LP_ALL) return bits;
                }
            }
        }
    }
    return bits;
}

__device__ __forceinline__ RowSeqs line_seqs(const DevGeo& L, int64_t i) {
    return L.type == GPK_GEOM_LINESTRING ? row_seqs<GPK_GEOM_LINESTRING>(L, i) : row_seqs<GPK_GEOM_MULTILINESTRING>(L, i);
}

// The walk itself: the mask of the coordinate sequences `l` (no NaN) against the usable polygon row `polys`[p0, p1) with the box of its
// shells.  `settled(mask)` ends the walk early (the mask is then partial).  The sequences of a line row — or the rings of another
// polygonal row taken as closed lines (gpk_polyrel.h).  Same value on every lane of the group.
template <int G, class Settled>
__device__ inline int sequences_mask_group(const RowSeqs& l, const DevGeo& polys, int p0, int p1, double4 box, int lane, Settled settled) {
    int mask = 0;
    for (int s = l.s0; s < l.s1; ++s) {
        const int c0 = l.so[s], c1 = l.so[s + 1];
        if (c1 <= c0) continue;
        double2 p = l.xy[c0];
        int pp = coord_bits<G>(polys, p0, p1, box, p, lane);
        mask |= pp;
        for (int c = c0 + 1; c < c1; ++c) {
            if (settled(mask)) return mask;
            const double2 q = l.xy[c];
            if (cont::same_xy(p, q)) continue;
            const int pq = coord_bits<G>(polys, p0, p1, box, q, lane);
            mask |= pq;
            if ((pp | pq) == (GPK_LP_INTERIOR | GPK_LP_EXTERIOR)) {
                mask |= GPK_LP_BOUNDARY;  // from the interior to the exterior: the segment meets a ring on the way
            } else if (!(fmax(p.x, q.x) < box.x || fmin(p.x, q.x) > box.z || fmax(p.y, q.y) < box.y || fmin(p.y, q.y) > box.w)) {
                if (pp == GPK_LP_BOUNDARY) mask |= side_bits<G>(polys, p0, p1, p, q, lane);
                if (pq == GPK_LP_BOUNDARY) mask |= side_bits<G>(polys, p0, p1, q, p, lane);
                if (!settled(mask)) mask |= segment_events<G>(polys, p0, p1, p, q, lane);
            }
            p = q;
            pp = pq;
        }
    }
    return mask;
}

// The mask of row i of `lines` (LINESTRING | MULTILINESTRING) against row j of `polys` (POLYGON | MULTIPOLYGON); rows out of range
// behave like null rows.  With `st` the walk ends as soon as the bits a caller needs are settled (the mask is then partial).
// Same value on every lane of the group.
template <int G>
__device__ inline int line_polygon_mask_group(const DevGeo& lines, int64_t i, const DevGeo& polys, int64_t j, int lane,
                                              Stop st = Stop{0, LP_ALL}) {
    if (!dev::row_ok(lines, i) || !dev::row_ok(polys, j)) return 0;
    const RowSeqs l = line_seqs(lines, i);
    if (l.c1 <= l.c0) return 0;
    {
        int nan = 0;
        for (int c = l.c0 + lane; c < l.c1; c += G) {
            const double2 v = l.xy[c];
            nan |= (v.x != v.x) | (v.y != v.y);
        }
        if (dev::group_or<G>(nan)) return 0;
    }
    int p0, p1;
    dev::geom_parts(polys, j, p0, p1);
    double4 box;
    if (!polygon_row_ok<G>(polys, p0, p1, lane, box)) return 0;
    return sequences_mask_group<G>(l, polys, p0, p1, box, lane, [st](int m) { return done(m, st); });
}

// lanes per pair: ring edges are what the lanes stride over, so the polygon column's mean coordinate count decides — about four
// edges per lane and round, rounded to the instantiated sizes 4 / 16; the line column's mean only sets how many rounds a pair takes
constexpr int LP_G_SMALL = 4, LP_G_LARGE = 16;
constexpr double LP_G_MEAN = 32.0;  // polygon rows of at least this many coordinates on average take LP_G_LARGE
static inline int relation_group_size(const DevGeo& lines, const DevGeo& polys) {
    (void)lines;
    const double m = polys.n_geoms > 0 ? (double)polys.n_coords / (double)polys.n_geoms : 0.0;
    return m >= LP_G_MEAN ? LP_G_LARGE : LP_G_SMALL;
}

}  // namespace lp
}  // namespace gpk
