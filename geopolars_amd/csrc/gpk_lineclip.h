// gpk_lineclip.h — the piece of a line inside (or outside) a polygonal geometry: gpk_line_clip (include/geopolars_hip.h; DESIGN.md
// section 4.3o).  L = a LINESTRING / MULTILINESTRING row, P = a POLYGON / MULTIPOLYGON row, P closed.
//   GPK_CLIP_INSIDE   L ∩ P: the pieces of L in P's interior or along a ring
//   GPK_CLIP_OUTSIDE  the closure of L \ P: the pieces of L in P's exterior (outside every part, or inside a hole)
// The result needs no ring reconstruction: it is a set of sub-intervals of L's own segments.
//
// Pieces.  Per coordinate sequence of L, in storage order.  A segment pq with p == q is skipped (q stays the previous distinct
// coordinate), so a repeated coordinate is never emitted twice.  The touch points of pq are those of gpk_linearea.h: an end on a ring,
// a ring vertex on the open segment, a proper crossing.  They cut pq into pieces, each INTERIOR, BOUNDARY (along a ring edge) or
// EXTERIOR, decided exactly: the piece next to a touch point that is a representable point (p, q, a ring vertex) by lp::side_bits
// against the whole geometry, the piece next to an end that lies on no ring by that end's position.  Kept: INTERIOR and BOUNDARY for
// INSIDE, EXTERIOR for OUTSIDE.
//
// Transitions.  A touch point or a vertex of L where the kept-ness of the piece before differs from that of the piece after.  Each
// carries its exact type, +1 (entry into kept) or -1 (exit):
//   a ring vertex v on the open segment   kept(side(v -> q)) - kept(side(v -> p)); 0: no transition, no trace in the output (a graze,
//                                         interior -> along an edge -> interior, touching from outside)
//   a proper crossing of ring edge ab     with no vertex of P at the crossing point the crossed ring is the only ring there and has one
//                                         side on either hand: always a transition, no side test.  q lies inside the ring iff
//                                         orient(a, b, q) * ccw > 0; inside a shell or outside a hole is INTERIOR.  With a vertex of P at
//                                         the crossing point (lp::vertex_at_crossing) that vertex is an event of the first kind of the
//                                         same segment and the crossing adds nothing.
// Parts.  A part is a maximal run of kept pieces within one sequence: the run's first point, every coordinate of L strictly inside
// the run, the run's last point.  Runs are not merged across the closing coordinate of a closed sequence nor across members; parts
// appear in the order the line is walked; a stretch the line covers twice is emitted twice (the convention of the length in
// gpk_overlay.h).
//
// Coordinates.  Every output coordinate is (a) a coordinate of L, bit for bit, (b) a vertex of P, bit for bit — a ring vertex on the
// open segment — or (c) a computed crossing p + t (q - p): t = |orient(a, b, p)| / (|orient(a, b, p)| + |orient(a, b, q)|) as floating
// determinants around a pair-local origin (the centre of the intersection of the two rows' boxes: at georeferenced magnitudes the
// determinants of raw coordinates lose every digit), clamped to [0, 1], the point clamped to the segment's box.  The point is on pq by
// construction and its distance to the carrier of ab is the error of t times |pq| sin(angle) — the angle cancels: within 1e-9 d of
// pq and of ab, d = the diagonal of the pair's joint box, whatever the crossing angle.  Near-parallel crossings move the point along
// both carriers, not off them.
//
// Order along a segment.  The run of a segment is assembled by walking its events in order (event_before):
//   two (b) points        exactly, by coordinate (equal coordinates are ONE touch point, taken once)
//   (b) against (c)       exactly: v lies before the crossing of ab iff orient(a, b, v) has the sign of orient(a, b, p)
//   two crossings         by their computed t (ties by edge number)
// The walk keeps a DEPTH, not a parity: depth = kept(piece at p) + the sum of the types passed so far, a piece is kept while
// depth > 0.  The sum of all types is exact whatever the order, so the state at q is the exact one, and two transitions closer than
// rounding that come out in the wrong order can only lose or create a piece shorter than the tolerance — they can never invert the
// rest of the segment.  The three exact rules and the computed t need not form one transitive order when events are closer than
// rounding; the walk is therefore bounded by the number of ring edges and always terminates.
//
// Contract.  If every two distinct transition points of a segment are at least 1e-6 |pq| apart, the parts and the coordinates per part
// are exactly those of the exact result ((a), (b) bit for bit, (c) within the bound above).  Below that gap the output's point set is
// within 1e-9 d (Hausdorff) of the exact one.  Invalid polygons: unspecified, the call terminates.
//
// Rows: a null row (validity 0) for every condition gpk_intersection_measure answers with NaN — either row null or out of range, no
// coordinate / no non-empty member, a ring that fails cont::ring_init, a NaN or infinite line coordinate.
//
// Schedule: G lanes per pair as in gpk_linearea.h — ring edges strided over the lanes, the segment and the event under test uniform in
// the group, every branch around a DPP reduction group-uniform.  No per-segment storage: from the current event the next one is found
// with one strided pass over the ring edges and a group minimum under event_before, so a segment costs (events + 1) x edges, one to
// three times the relation walk on ordinary data.  A segment whose box misses the box of P's shells is one EXTERIOR piece.  Rows of
// many thousand coordinates run on the same lanes: correct and slow.
//
// The arithmetic that is new here — the crossing point, the order of events and the run state machine — is plain C++ over an Orient
// parameter, as in gpk_overlay.h: tests/lineclip_host_driver.cpp runs it on the CPU.  The group routine on top is device code; the
// count pass and the fill pass instantiate it with two sinks, so both make bit-identical decisions.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GPK_LC_FN __host__ __device__ inline
#else
#define GPK_LC_FN inline
#endif

namespace gpk {
namespace lc {

struct P2 {
    double x, y;
};

constexpr int MODE_INSIDE = 0, MODE_OUTSIDE = 1;
constexpr int CLS_INTERIOR = 1, CLS_BOUNDARY = 2, CLS_EXTERIOR = 4;  // the bits of GPK_LP_*

GPK_LC_FN bool kept(int cls, int mode) { return mode == MODE_INSIDE ? (cls & (CLS_INTERIOR | CLS_BOUNDARY)) != 0 : cls == CLS_EXTERIOR; }

// the parameter of the proper crossing of p -> q with the carrier of ab, around the local origin o
GPK_LC_FN double crossing_t(P2 p, P2 q, P2 a, P2 b, P2 o) {
    const double ax = a.x - o.x, ay = a.y - o.y;
    const double ex = (b.x - o.x) - ax, ey = (b.y - o.y) - ay;
    const double da = fabs(ex * ((p.y - o.y) - ay) - ey * ((p.x - o.x) - ax));
    const double db = fabs(ex * ((q.y - o.y) - ay) - ey * ((q.x - o.x) - ax));
    const double s = da + db;
    const double t = s > 0.0 ? da / s : 0.5;
    return fmin(1.0, fmax(0.0, t));
}
// p + t (q - p), kept inside the segment's box
GPK_LC_FN P2 point_at(P2 p, P2 q, double t) {
    const double x = p.x + t * (q.x - p.x), y = p.y + t * (q.y - p.y);
    return P2{fmin(fmax(p.x, q.x), fmax(fmin(p.x, q.x), x)), fmin(fmax(p.y, q.y), fmax(fmin(p.y, q.y), y))};
}

// An event of segment pq.  kind 0: the ring vertex a on the open segment (a (b) point); kind 1: the proper crossing with ring edge
// ab at parameter t; kind -1: "before every event".  id: unique per event of a row (2 x the coordinate number of a, + kind).
struct Event {
    int kind, id;
    P2 a, b;
    double t;
};

// does e come strictly before f on p -> q.  orient(u, v, w): the exact sign of cross(v - u, w - u).
template <class Orient>
GPK_LC_FN bool event_before(const Event& e, const Event& f, P2 p, P2 q, Orient orient) {
    if (e.kind < 0) return f.kind >= 0;
    if (f.kind < 0) return false;
    if (e.kind == 0 && f.kind == 0) {  // both on the carrier of pq: any coordinate that changes along it orders them exactly
        if (p.x != q.x) return q.x > p.x ? e.a.x < f.a.x : e.a.x > f.a.x;
        return q.y > p.y ? e.a.y < f.a.y : e.a.y > f.a.y;
    }
    if (e.kind == 0) {  // vertex against crossing; a vertex AT the crossing point comes first (the crossing is then dropped)
        const int s = orient(f.a, f.b, e.a);
        return s == 0 || s == orient(f.a, f.b, p);
    }
    if (f.kind == 0) {
        const int s = orient(e.a, e.b, f.a);
        return s != 0 && s != orient(e.a, e.b, p);
    }
    return e.t < f.t || (e.t == f.t && e.id < f.id);
}

// The earlier of two events given by value (the reduction step of the search for the next event); symmetric in its arguments whatever
// event_before answers, so a butterfly over lanes leaves the same event on all of them.
template <class Orient>
GPK_LC_FN const Event& earlier(const Event& e, const Event& f, P2 p, P2 q, Orient orient) {
    if (e.kind < 0) return f;
    if (f.kind < 0 || e.id == f.id) return e;
    const Event &lo = e.id < f.id ? e : f, &hi = e.id < f.id ? f : e;
    return event_before(lo, hi, p, q, orient) ? lo : hi;
}

// The type of a proper crossing with no vertex of P at the crossing point: +1 entry into kept, -1 exit.  side_q = orient(a, b, q),
// ccw = the ring's winding (+1 / -1), hole: the ring is a hole of its member.
GPK_LC_FN int crossing_type(int side_q, int ccw, bool hole, int mode) {
    const bool q_in_ring = side_q * ccw > 0;
    const int after = q_in_ring != hole ? CLS_INTERIOR : CLS_EXTERIOR, before = q_in_ring != hole ? CLS_EXTERIOR : CLS_INTERIOR;
    return (kept(after, mode) ? 1 : 0) - (kept(before, mode) ? 1 : 0);
}

// The run state machine of one coordinate sequence.  Sink: begin_part() opens a part, coord(P2) appends a coordinate to the open part.
struct Run {
    int depth;  // kept(piece at p) + the types passed so far on the current segment
    bool open;  // a part is open (its last coordinate so far is the last one handed to the sink)
};
GPK_LC_FN Run run_start() { return Run{0, false}; }
// segment p -> q begins; kept0: the piece next to p is kept.  A run that was open and does not go on ended at p, which it holds.
template <class Sink>
GPK_LC_FN void run_segment_begin(Run& r, bool kept0, P2 p, Sink& out) {
    if (kept0 && !r.open) {
        out.begin_part();
        out.coord(p);
    }
    r.open = kept0;
    r.depth = kept0 ? 1 : 0;
}
// an event of type `type` (+1, -1) at the point x
template <class Sink>
GPK_LC_FN void run_transition(Run& r, int type, P2 x, Sink& out) {
    const bool before = r.depth > 0;
    r.depth += type;
    const bool after = r.depth > 0;
    if (!before && after) out.begin_part();
    if (before != after) out.coord(x);
    r.open = after;
}
// the segment ends at q
template <class Sink>
GPK_LC_FN void run_segment_end(Run& r, P2 q, Sink& out) {
    r.open = r.depth > 0;
    if (r.open) out.coord(q);
}

// the pair-local origin: the centre of the intersection of the two rows' boxes (of the joint box when they are apart)
GPK_LC_FN P2 local_origin(double ax0, double ay0, double ax1, double ay1, double bx0, double by0, double bx1, double by1) {
    return P2{0.5 * fmax(ax0, bx0) + 0.5 * fmin(ax1, bx1), 0.5 * fmax(ay0, by0) + 0.5 * fmin(ay1, by1)};
}

}  // namespace lc
}  // namespace gpk

#if defined(__HIPCC__)
// ---- the device group routine -----------------------------------------------------------------------------------------------------
#include "gpk_linearea.h"

namespace gpk {
namespace lc {

struct DevOrient {
    __device__ __forceinline__ int operator()(P2 a, P2 b, P2 c) const { return dev::orient2d(a.x, a.y, b.x, b.y, c.x, c.y); }
};
__device__ __forceinline__ P2 p2(double2 v) { return P2{v.x, v.y}; }

constexpr int NO_EVENT = 0x7fffffff;

// the event `id` of segment pq, rebuilt from the row's coordinates: every lane that holds an id holds the same event
__device__ __forceinline__ Event event_of(int id, const double2* __restrict__ xy, P2 p, P2 q, P2 o) {
    Event e;
    e.kind = id == NO_EVENT ? -1 : (id & 1);
    e.id = id;
    e.t = 0.0;
    if (id == NO_EVENT) {
        e.a = e.b = p;
        return e;
    }
    e.a = p2(xy[id >> 1]);
    e.b = p2(xy[(id >> 1) + 1]);
    if (e.kind == 1) e.t = crossing_t(p, q, e.a, e.b, o);
    return e;
}

// The first event of segment pq (p != q) strictly after `cur` (NO_EVENT: the first of all), NO_EVENT when there is none.  One strided
// pass over the ring edges of the usable row, then the group minimum.  Same value on every lane.
template <int G>
__device__ inline int next_event(const DevGeo& P, int p0, int p1, double2 p, double2 q, P2 o, int cur, int lane) {
    const double lx = fmin(p.x, q.x), hx = fmax(p.x, q.x), ly = fmin(p.y, q.y), hy = fmax(p.y, q.y);
    const P2 pp = p2(p), qq = p2(q);
    const Event ec = event_of(cur, P.xy, pp, qq, o);
    Event best = event_of(NO_EVENT, P.xy, pp, qq, o);
    for (int pt = p0; pt < p1; ++pt) {
        int r0, r1;
        if (!lp::part_of(P, pt, r0, r1)) continue;
        for (int r = r0; r < r1; ++r) {
            const int c0 = P.ring_off[r], m = P.ring_off[r + 1] - c0 - 1;
            for (int i = lane; i < m; i += G) {
                const int ev = lp::edge_events(p, q, lx, hx, ly, hy, P.xy[c0 + i], P.xy[c0 + i + 1]);
                for (int k = 0; k < 2; ++k) {
                    if (!(ev & (1 << k))) continue;
                    const Event e = event_of(2 * (c0 + i) + k, P.xy, pp, qq, o);
                    if (!event_before(ec, e, pp, qq, DevOrient{})) continue;
                    best = earlier(best, e, pp, qq, DevOrient{});
                }
            }
        }
    }
    return dev::group_allreduce<G>(best.id, [&](int a, int b) {
        return earlier(event_of(a, P.xy, pp, qq, o), event_of(b, P.xy, pp, qq, o), pp, qq, DevOrient{}).id;
    });
}

// the ring of the usable row that holds coordinate c: its winding, and whether it is a hole of its member
template <int G>
__device__ inline void ring_of(const DevGeo& P, int p0, int p1, int c, int lane, int& ccw, bool& hole) {
    ccw = 1;
    hole = false;
    for (int pt = p0; pt < p1; ++pt) {
        int r0, r1;
        if (!lp::part_of(P, pt, r0, r1)) continue;
        for (int r = r0; r < r1; ++r) {
            const int c0 = P.ring_off[r], n = P.ring_off[r + 1] - c0;
            if (c < c0 || c >= c0 + n) continue;
            cont::Ring R;
            (void)cont::ring_init<G>(R, P.xy + c0, n, lane);
            ccw = R.ccw;
            hole = r > r0;
            return;
        }
    }
}

// The clip of row i of `lines` against row j of `polys` into `out` (begin_part / coord, called with the same arguments on every lane
// of the group).  Returns false for a null result row.
template <int G, class Sink>
__device__ inline bool clip_group(const DevGeo& lines, int64_t i, const DevGeo& polys, int64_t j, int mode, int lane, Sink& out) {
    if (i < 0 || j < 0 || !dev::row_ok(lines, i) || !dev::row_ok(polys, j)) return false;
    const RowSeqs l = lp::line_seqs(lines, i);
    if (l.c1 <= l.c0) return false;
    double4 box_l;
    {
        int bad = 0;
        double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
        for (int c = l.c0 + lane; c < l.c1; c += G) {
            const double2 v = l.xy[c];
            bad |= (fabs(v.x) < INFINITY && fabs(v.y) < INFINITY) ? 0 : 1;  // NaN or infinite
            mnx = fmin(mnx, v.x); mny = fmin(mny, v.y); mxx = fmax(mxx, v.x); mxy = fmax(mxy, v.y);
        }
        if (dev::group_or<G>(bad)) return false;
        box_l = make_double4(dev::group_min<G>(mnx), dev::group_min<G>(mny), dev::group_max<G>(mxx), dev::group_max<G>(mxy));
    }
    int p0, p1;
    dev::geom_parts(polys, j, p0, p1);
    double4 box;
    if (!lp::polygon_row_ok<G>(polys, p0, p1, lane, box)) return false;
    const P2 o = local_origin(box_l.x, box_l.y, box_l.z, box_l.w, box.x, box.y, box.z, box.w);
    const int32_t* part_ring = polys.type == GPK_GEOM_MULTIPOLYGON ? polys.part_off : polys.geom_off;
    const int row_c0 = polys.ring_off[part_ring[p0]], row_c1 = polys.ring_off[part_ring[p1]];  // the row's coordinates are contiguous
    const int max_events = 2 * (row_c1 - row_c0);

    for (int s = l.s0; s < l.s1; ++s) {
        const int c0 = l.so[s], c1 = l.so[s + 1];
        if (c1 <= c0) continue;
        Run run = run_start();
        double2 p = l.xy[c0];
        int pp = lp::coord_bits<G>(polys, p0, p1, box, p, lane);
        for (int c = c0 + 1; c < c1; ++c) {
            const double2 q = l.xy[c];
            if (cont::same_xy(p, q)) continue;
            const int pq = lp::coord_bits<G>(polys, p0, p1, box, q, lane);
            // the piece next to p: where p lies, or — p on a ring — where the segment leaves it (then p is in the box, and so is pq's)
            const int first = pp == GPK_LP_BOUNDARY ? lp::side_bits<G>(polys, p0, p1, p, q, lane) : pp;
            run_segment_begin(run, kept(first, mode), p2(p), out);
            const double lx = fmin(p.x, q.x), hx = fmax(p.x, q.x), ly = fmin(p.y, q.y), hy = fmax(p.y, q.y);
            if (!(hx < box.x || lx > box.z || hy < box.y || ly > box.w)) {
                int cur = NO_EVENT;
                for (int it = 0; it < max_events; ++it) {
                    cur = next_event<G>(polys, p0, p1, p, q, o, cur, lane);
                    if (cur == NO_EVENT) break;
                    const Event e = event_of(cur, polys.xy, p2(p), p2(q), o);
                    const double2 a = make_double2(e.a.x, e.a.y), b = make_double2(e.b.x, e.b.y);
                    if (e.kind == 0) {
                        const int after = lp::side_bits<G>(polys, p0, p1, a, q, lane), before = lp::side_bits<G>(polys, p0, p1, a, p, lane);
                        const int type = (kept(after, mode) ? 1 : 0) - (kept(before, mode) ? 1 : 0);
                        if (type) run_transition(run, type, e.a, out);
                    } else if (!lp::vertex_at_crossing<G>(polys.xy, row_c0, row_c1, p, q, lx, hx, ly, hy, a, b, lane)) {
                        int ccw;
                        bool hole;
                        ring_of<G>(polys, p0, p1, cur >> 1, lane, ccw, hole);
                        run_transition(run, crossing_type(cont::orient(a, b, q), ccw, hole, mode), point_at(p2(p), p2(q), e.t), out);
                    }
                }
            }
            run_segment_end(run, p2(q), out);
            p = q;
            pp = pq;
        }
    }
    return true;
}

}  // namespace lc
}  // namespace gpk
#endif
