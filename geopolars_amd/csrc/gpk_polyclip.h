// gpk_polyclip.h — the geometry two polygonal rows share, or the part of the first outside the second: gpk_polygon_clip
// (include/geopolars_hip.h).  a, b = POLYGON / MULTIPOLYGON rows.
//   GPK_PCLIP_INTERSECTION  the closure of int(a) ∩ int(b)
//   GPK_PCLIP_DIFFERENCE    the closure of int(a) \ b
// Both are REGULARISED: the area part only.  Points and edges the operands merely share leave no trace.
//
// Rule 1, walks.  Every ring of a row is walked with the row's interior on its left: shells counter-clockwise, holes clockwise.  A ring
// stored the other way (the winding cont::ring_init gives) is walked backwards.  A segment pq with p == q is skipped, as in the line
// clip.
//
// Rule 2, kept pieces.  Touch points, the piece classes INTERIOR / BOUNDARY / EXTERIOR, transition types and the depth walk are those of
// gpk_lineclip.h, the walked ring taking the place of the line and the other row that of the polygon.  One addition: a BOUNDARY piece
// runs along an edge of the other row, and what matters is whether that row's interior lies on the SAME side of the piece (its left) or
// on the OPPOSITE side.  boundary_class decides it exactly from the direction of the carrying edge, its ring's winding and its hole flag.
//     walk              INTERSECTION keeps               DIFFERENCE keeps
//     ∂a against b      INTERIOR; BOUNDARY same side     EXTERIOR; BOUNDARY opposite side
//     ∂b against a      INTERIOR only                    INTERIOR only, emitted backwards
// Shared boundary always comes from a, never from b: equal polygons intersect to a, a polygon minus itself is empty, neighbours that
// share an edge intersect to nothing.
//
// Rule 3, arcs.  A maximal kept run is a directed arc with the result on its left; runs ARE merged across the closing coordinate of a
// ring (the ring is walked once, and a second time up to the first arc end when its first piece is kept).  The two ends of an arc carry
// exact identities: an input coordinate carries its value (End::ea < 0), a proper crossing the pair (edge of a, edge of b), each edge
// named by the number of its first coordinate in its column.  A crossing has ONE coordinate value wherever it is emitted:
// lc::point_at along the edge of a in storage order with lc::crossing_t against the edge of b in storage order (crossing_point), in
// both walks — the walk over ∂b orders its events by the parameter along b's edge but emits a's value — moved by ulps onto the closed
// inner side of a's edge, so that the exact relation of a result to a is covered-by, and where an end of one edge lies within ulps of
// the other edge to a double that leaves every end on its own side of the emitted half edges (crossing_keeps_sides): the ring does
// not fold over an ulp at a vertex next to a crossing.  Arcs are linked by identity,
// never by comparing computed coordinates; a ring is closed when the walk returns to its first arc.
//
// Rule 4, junctions.  More than one arc can end at the same point only at an input coordinate, where rings touch.  There the
// continuation of an incoming arc is the first outgoing arc met when turning clockwise from the direction it came from: the leftmost
// turn (cw_before), chosen with exact orientation signs of input coordinates only — the neighbour of a computed crossing is replaced by
// the far end of its edge (Arc::s_nb, Arc::e_nb).  So that every point where rings of the result can touch IS an arc end, a kept run
// is also CUT, without a transition, where it merely touches the other row's boundary at an input coordinate: the pieces before and
// after both kept and both INTERIOR or both EXTERIOR (is_cut) — at a vertex of the walked ring that lies on the other row's boundary,
// or at a vertex of the other row on the open segment, which thereby becomes a coordinate of the result.  A ring with neither a
// transition nor a cut is kept whole or dropped whole.  Consequences:
//   - parts of the result that touch at a point stay separate rings;
//   - a hole that touches its shell at a point fuses into the shell, which then touches itself there: status 1, the only case in
//     which gpk_validity may object to an output row (b inside a and touching it from within at a point: a \ b is ONE ring that passes
//     twice through that point).
//
// Rule 5, rings to polygons.  The sign of a ring is exact: at its lexicographically lowest point the lowest-lying incident edge is an
// outgoing one for a counter-clockwise ring (ring_sign), in orientation signs of INPUT coordinates only — the directions of the
// edges at that point are taken from the ends of their carrying segments, never from a computed crossing; positive: a shell,
// negative: a hole; a degenerate sign gives status 4 and cannot occur above the gap.  A ring starts at its arc with the smallest key
// (walk of a before walk of b, then the number of the segment its arc starts on, an arc that starts at the segment's first coordinate
// before one that starts inside it).  Parts are ordered by their shell's key; each hole goes to the first shell in key order that
// encloses it.  Enclosure (ring_encloses) is the exact crossing-number test of the first coordinate of the hole that is an input
// coordinate and not on the shell; when the hole has no such coordinate the first computed crossing off the shell is tested in the
// same way — exact for the double that is emitted, which lies within 1e-9 d of the exact crossing; a hole none of whose coordinates is
// off the candidate is not enclosed by it.  Output rings are closed, shells counter-clockwise, holes clockwise.
//
// Rule 6, contract.  Every output coordinate is a coordinate of a, bit for bit, a coordinate of b, bit for bit, or a crossing within
// 1e-9 d of both carrying edges, d = the diagonal of the pair's joint box (the line clip's bound with the same arithmetic around the
// same pair-local origin).  If every two distinct transition points on a segment are at least 1e-6 |segment| apart, then parts, rings,
// coordinates per ring and ring starts are those of the exact result.  Below the gap either the point set is within 1e-9 d of the
// exact one or the row has status 4 (the arcs did not close into rings, a ring without a sign, a hole without a shell): the row is
// then null, never a guessed geometry.  Invalid polygons: unspecified, the call terminates (every loop is bounded by the number of
// edges or arcs).  A proper crossing of an edge of a with an edge of b exactly at a vertex of another ring of either row (rings of a
// valid row may touch there) carries that vertex as its identity and value in both walks.
// The result is identical at every placement, for every lane-group size and on every schedule.
//
// Schedule: G lanes per pair (lp::relation_group_size; 4 and 16), ring edges strided over the lanes, every branch around a DPP
// reduction group-uniform, as gpk_lineclip.h.  The stitch of a pair's arcs is sequential and runs on the first lane of the group.  Rows
// of many thousand coordinates run on the same lanes: correct and slow.
//
// What is new here — the kept table, the side of a shared edge, the arc state machine, the junction order and the stitcher from arc
// records to rings, signs and nesting — is plain C++ over an Orient parameter: tests/polyclip_host_driver.cpp runs it on the CPU.
#pragma once

#include "gpk_lineclip.h"

namespace gpk {
namespace pc {

using lc::P2;

constexpr int MODE_INTERSECTION = 0, MODE_DIFFERENCE = 1;
constexpr int WALK_A = 0, WALK_B = 1;
constexpr int CLS_INTERIOR = 1, CLS_BOUNDARY_SAME = 2, CLS_EXTERIOR = 4, CLS_BOUNDARY_OPP = 8;
constexpr int ST_OK = 0, ST_TOUCH = 1, ST_EMPTY = 2, ST_NULL = 3, ST_UNRESOLVED = 4;

// the kept table of rule 2
GPK_LC_FN bool kept(int cls, int walk, int mode) {
    if (walk == WALK_B) return cls == CLS_INTERIOR;
    return mode == MODE_INTERSECTION ? (cls & (CLS_INTERIOR | CLS_BOUNDARY_SAME)) != 0 : (cls & (CLS_EXTERIOR | CLS_BOUNDARY_OPP)) != 0;
}
// arcs of ∂b bound a \ b with the result on their RIGHT: they are emitted backwards
GPK_LC_FN bool emitted_backwards(int walk, int mode) { return walk == WALK_B && mode == MODE_DIFFERENCE; }
// The two tables as a type.  The crossing type, the cut test and the device walks take any rule of this shape (gpk_polyunion.h has
// another one); without one they take this, and compile to what they were.
struct ClipRule {
    static constexpr bool DIRECTION_BY_CLASS = false;  // a walk is emitted one way throughout (gpk_polysymdiff.h has the other kind)
    static GPK_LC_FN bool kept(int cls, int walk, int mode) { return pc::kept(cls, walk, mode); }
    static GPK_LC_FN bool emitted_backwards(int walk, int mode) { return pc::emitted_backwards(walk, mode); }
};

// The class of a piece t -> w that runs along the edge a -> b (storage order) of the other row; ccw: the winding of the edge's ring,
// hole: the ring is a hole of its member.  The other row's interior lies left of a -> b iff the ring is a ccw shell or a cw hole.
GPK_LC_FN int boundary_class(P2 a, P2 b, P2 t, P2 w, int ccw, bool hole) {
    const bool left_of_edge = (ccw > 0) != hole;
    const bool same_dir = a.x != b.x ? (b.x > a.x) == (w.x > t.x) : (b.y > a.y) == (w.y > t.y);
    return left_of_edge == same_dir ? CLS_BOUNDARY_SAME : CLS_BOUNDARY_OPP;
}

// the class of a piece that was judged looking BACK along the walk (from a touch point towards p): the sides change hands
GPK_LC_FN int looking_back(int cls) { return cls == CLS_BOUNDARY_SAME ? CLS_BOUNDARY_OPP : (cls == CLS_BOUNDARY_OPP ? CLS_BOUNDARY_SAME : cls); }

// The type of a proper crossing with no vertex at the crossing point (lc::crossing_type with this kept table)
template <class Rule>
GPK_LC_FN int crossing_type_by(int side_q, int ccw, bool hole, int walk, int mode) {
    const bool q_in_ring = side_q * ccw > 0;
    const int after = q_in_ring != hole ? CLS_INTERIOR : CLS_EXTERIOR, before = q_in_ring != hole ? CLS_EXTERIOR : CLS_INTERIOR;
    return (Rule::kept(after, walk, mode) ? 1 : 0) - (Rule::kept(before, walk, mode) ? 1 : 0);
}
GPK_LC_FN int crossing_type(int side_q, int ccw, bool hole, int walk, int mode) { return crossing_type_by<ClipRule>(side_q, ccw, hole, walk, mode); }

// Does the emitted crossing x leave every end of either edge on the side it is on?  The result's edges at a crossing are the halves
// x -> end of the two crossing edges.  An end of the OTHER edge that lies an ulp from this edge's carrier (a vertex next to the
// crossing) can come to lie on the wrong side of an emitted half although it is on the right side of the edge itself: the ring then
// folds over that ulp and is no valid polygon.  Exact signs of doubles.
template <class Orient>
GPK_LC_FN bool crossing_keeps_sides(P2 x, P2 a0, P2 a1, P2 b0, P2 b1, Orient orient) {
    const P2 u[2] = {a0, b0}, v[2] = {a1, b1}, e0[2] = {b0, a0}, e1[2] = {b1, a1};
    for (int k = 0; k < 2; ++k)
        for (int j = 0; j < 2; ++j) {
            const P2 e = j ? e1[k] : e0[k];
            const bool ex = e.x == x.x && e.y == x.y;
            const int s = orient(u[k], v[k], e);
            if (!ex && !(x.x == v[k].x && x.y == v[k].y) && !(e.x == v[k].x && e.y == v[k].y) && orient(x, v[k], e) != s) return false;
            if (!ex && !(x.x == u[k].x && x.y == u[k].y) && !(e.x == u[k].x && e.y == u[k].y) && orient(u[k], x, e) != s) return false;
        }
    return true;
}
GPK_LC_FN double ulps_away(double v, int k) {
    for (; k > 0; --k) v = nextafter(v, INFINITY);
    for (; k < 0; ++k) v = nextafter(v, -INFINITY);
    return v;
}

// The one coordinate value of the crossing of edge a0 -> a1 of a with edge b0 -> b1 of b (storage order both), around the origin o.
// a_left: a's interior lies left of a0 -> a1.  The rounded point is then moved, an ulp of one coordinate at a time, onto the closed
// inner side of a's edge (exact signs; it starts within a few ulps of the edge), so that no vertex of a result lies outside a.  Where
// that point fails crossing_keeps_sides — only when an end of one edge lies within ulps of the other edge — the doubles up to
// CROSSING_SEARCH ulps around it are tried, nearest ring first, for one on a's closed inner side and in a's box that keeps the sides;
// without one the point stays (the row is then within 1e-9 d all the same, and may be no valid polygon).
constexpr int CROSSING_SEARCH = 3;
template <class Orient>
GPK_LC_FN P2 crossing_point(P2 a0, P2 a1, P2 b0, P2 b1, P2 o, bool a_left, Orient orient) {
    P2 x = lc::point_at(a0, a1, lc::crossing_t(a0, a1, b0, b1, o));
    const double nx = a_left ? a0.y - a1.y : a1.y - a0.y, ny = a_left ? a1.x - a0.x : a0.x - a1.x;  // the inward normal
    const int want = a_left ? 1 : -1;
    for (int it = 0; it < 8; ++it) {
        const int s = orient(a0, a1, x);
        if (s == 0 || s == want) break;
        if (fabs(nx) >= fabs(ny))
            x.x = nextafter(x.x, nx > 0.0 ? INFINITY : -INFINITY);
        else
            x.y = nextafter(x.y, ny > 0.0 ? INFINITY : -INFINITY);
    }
    if (crossing_keeps_sides(x, a0, a1, b0, b1, orient)) return x;
    const double lx = fmin(a0.x, a1.x), hx = fmax(a0.x, a1.x), ly = fmin(a0.y, a1.y), hy = fmax(a0.y, a1.y);
    for (int r = 1; r <= CROSSING_SEARCH; ++r)
        for (int dx = -r; dx <= r; ++dx)
            for (int dy = -r; dy <= r; ++dy) {
                if (dx != -r && dx != r && dy != -r && dy != r) continue;
                const P2 y{ulps_away(x.x, dx), ulps_away(x.y, dy)};
                if (y.x < lx || y.x > hx || y.y < ly || y.y > hy) continue;
                const int s = orient(a0, a1, y);
                if ((s == 0 || s == want) && crossing_keeps_sides(y, a0, a1, b0, b1, orient)) return y;
            }
    return x;
}

// ---- arcs ------------------------------------------------------------------------------------------------------------------------
struct End {
    double x, y;  // the coordinate that is emitted
    int ea, eb;   // ea < 0: an input coordinate, identified by (x, y); else the crossing of edge ea of a with edge eb of b
    P2 far;       // an end INSIDE a segment p -> q of its walk (a crossing, a vertex of the other row): the segment's other end — p
                  // behind the start of an arc, q beyond its end, in the emitted direction; set by the run routines below, which know
                  // the segment.  (An end at a coordinate of the walked ring holds its own value here; ring_corners copies it and
                  // nothing reads the copy, since such a corner is not `computed`.)  At a crossing every arc end has its OWN far:
                  // under the clip's and the union's rules one arc ends and one starts there; under a rule with directions by class
                  // two end and two start (turn_to), the two of a walk with the two ends of that walk's segment, and stitch<true>
                  // reads e.far of the arriving arc for the leftmost turn.
};
GPK_LC_FN End end_at_coord(P2 v) { return End{v.x, v.y, -1, -1, v}; }
GPK_LC_FN End with_far(End id, P2 far) {
    id.far = far;
    return id;
}
GPK_LC_FN bool same_end(const End& u, const End& v) {
    return u.ea < 0 ? (v.ea < 0 && u.x == v.x && u.y == v.y) : (u.ea == v.ea && u.eb == v.eb);
}

constexpr int ARC_WHOLE = 1;      // a ring kept whole: closed in itself, no links
constexpr int ARC_BACKWARDS = 2;  // stored in walk order, emitted backwards (s, e, s_nb, e_nb are those of the emitted direction)
constexpr int KEY_WALK_B = 1 << 30;

struct Arc {
    End s, e;       // the ends, in the emitted direction
    P2 s_nb, e_nb;  // the input coordinates that give the direction of departure from s and the direction of arrival at e
    int c0, len;    // the arc's coordinates in the arc coordinate store, both ends included (len >= 2)
    int key;        // (walk << 30) | 2 * (segment of the start, counted in walk order from the row's first coordinate) | starts inside it
    int flags;
};

GPK_LC_FN P2 arc_coord(const Arc& a, const P2* xy, int j) { return xy[(a.flags & ARC_BACKWARDS) ? a.c0 + a.len - 1 - j : a.c0 + j]; }

// The arc state machine of one ring walk (lc::Run made cyclic).  Sink: begin_arc(End, P2 s_nb, int key), coord(P2),
// end_arc(End, P2 e_nb, int flags).  The piece at the ring's first coordinate has no piece before it on the first lap: when it is kept
// it is a HEAD, walked silently, and handed to the sink on the second lap, where the state before it is known.
struct Run {
    int depth;      // kept(piece at p) + the types passed so far on the current segment
    bool open;      // a kept run is open
    bool emit;      // ... and the sink has it (false: the silent head)
    bool head;      // the first piece of the ring is kept
    bool any_break; // an arc has ended: an exit or a cut
    bool started;   // the first segment has begun
    bool stop;      // second lap: the next break ends the walk (no arc begins there)
    P2 prev_p;      // the first coordinate of the segment before the current one (the direction of arrival at the current p)
};
GPK_LC_FN Run run_start() { return Run{0, false, false, false, false, false, false, P2{0.0, 0.0}}; }

// is a touch point that is no transition a CUT: both pieces kept and neither along an edge of the other row
template <class Rule>
GPK_LC_FN bool is_cut_by(int cls_before, int cls_after, int walk, int mode) {
    return Rule::kept(cls_after, walk, mode) && Rule::kept(cls_before, walk, mode) && (cls_before & (CLS_INTERIOR | CLS_EXTERIOR)) != 0 &&
           (cls_after & (CLS_INTERIOR | CLS_EXTERIOR)) != 0;
}
GPK_LC_FN bool is_cut(int cls_before, int cls_after, int walk, int mode) { return is_cut_by<ClipRule>(cls_before, cls_after, walk, mode); }
// A cut of the open run at the input coordinate `id` of segment p -> q; inside: strictly inside the segment (else at p).  Not a
// transition: the depth stays.
template <class Sink>
GPK_LC_FN void run_cut(Run& r, End id, bool inside, P2 p, P2 q, int seg, int walk, Sink& out) {
    if (!r.open) return;
    if (r.emit) {
        if (inside) out.coord(P2{id.x, id.y});
        out.end_arc(with_far(id, q), inside ? p : r.prev_p, 0);
    }
    r.any_break = true;
    r.emit = false;
    if (r.stop) {
        r.open = false;
        return;
    }
    out.begin_arc(with_far(id, p), q, (walk == WALK_B ? KEY_WALK_B : 0) | (2 * seg + (inside ? 1 : 0)));
    out.coord(P2{id.x, id.y});
    r.emit = true;
}

// segment p -> q (number `seg` of the walk) begins; kept0: the piece next to p is kept
template <class Sink>
GPK_LC_FN void run_segment_begin(Run& r, bool kept0, P2 p, P2 q, int seg, int walk, Sink& out) {
    if (!r.started) {
        r.started = true;
        r.head = kept0;
        r.open = kept0;
        r.emit = false;
        r.depth = kept0 ? 1 : 0;
        return;
    }
    if (r.open && !kept0) {
        if (r.emit) out.end_arc(end_at_coord(p), r.prev_p, 0);
        r.any_break = true;
        r.emit = false;
    } else if (!r.open && kept0) {
        out.begin_arc(end_at_coord(p), q, (walk == WALK_B ? KEY_WALK_B : 0) | (2 * seg));
        out.coord(p);
        r.emit = true;
    }
    r.open = kept0;
    r.depth = kept0 ? 1 : 0;
}
// an event of type `type` (+1, -1) with the identity `id` on segment p -> q
template <class Sink>
GPK_LC_FN void run_transition(Run& r, int type, End id, P2 p, P2 q, int seg, int walk, Sink& out) {
    const bool before = r.depth > 0;
    r.depth += type;
    const bool after = r.depth > 0;
    if (!before && after) {
        out.begin_arc(with_far(id, p), q, (walk == WALK_B ? KEY_WALK_B : 0) | (2 * seg + 1));
        out.coord(P2{id.x, id.y});
        r.emit = true;
    } else if (before && !after) {
        if (r.emit) {
            out.coord(P2{id.x, id.y});
            out.end_arc(with_far(id, q), p, 0);
        }
        r.any_break = true;
        r.emit = false;
    }
    r.open = after;
}
// the segment p -> q ends
template <class Sink>
GPK_LC_FN void run_segment_end(Run& r, P2 p, P2 q, Sink& out) {
    r.open = r.depth > 0;
    if (r.open && r.emit) out.coord(q);
    r.prev_p = p;
}

// ---- the same machine under a rule whose DIRECTION goes by class (Rule::DIRECTION_BY_CLASS; gpk_polysymdiff.h) -------------------------
// Such a rule keeps INTERIOR and EXTERIOR pieces alike and emits the INTERIOR ones backwards, so a kept run does not only begin and
// end: it TURNS where the class changes, and an arc ends and another begins there with the same identity.  Run::depth is then the
// LEVEL of the walk inside the other row — 1 for an INTERIOR piece at an exact class (a segment's begin, an input coordinate), 0 for
// an EXTERIOR one, +1 / -1 at every proper crossing — and a kept piece is emitted backwards while the level is positive: as with
// the depth above, two crossings closer than rounding that come out in the wrong order cannot invert the rest of the segment.
// The sink has one more call, rekey(int key), made before end_arc of a backwards arc: the key of an arc is that of its start in the
// EMITTED direction, which a backwards arc reaches last — the segment the walk is on when the arc ends, | 1 when it ends inside it.
// A forwards and a backwards arc that start at the same point of the same walk thus share a key; the backwards one has ended
// there, so it has the lower arc number and comes first (key_less).
GPK_LC_FN int arc_key(int walk, int seg, bool inside) { return (walk == WALK_B ? KEY_WALK_B : 0) | (2 * seg + (inside ? 1 : 0)); }
GPK_LC_FN int level_of(int cls) { return cls == CLS_INTERIOR ? 1 : 0; }
// the class after a proper crossing with no vertex at the crossing point (the first half of crossing_type_by)
GPK_LC_FN int class_after_crossing(int side_q, int ccw, bool hole) { return ((side_q * ccw > 0) != hole) ? CLS_INTERIOR : CLS_EXTERIOR; }

// the open arc ends at `id` on segment p -> q (inside: strictly inside it, else at p)
template <class Sink>
GPK_LC_FN void turn_close(Run& r, End id, bool inside, P2 p, P2 q, int key, Sink& out) {
    if (r.emit) {
        const bool back = r.depth > 0;
        if (inside) out.coord(P2{id.x, id.y});
        if (back) out.rekey(key);
        out.end_arc(with_far(id, q), inside ? p : r.prev_p, back ? ARC_BACKWARDS : 0);
    }
    r.any_break = true;
    r.emit = false;
}
// The piece after `id` is kept or not (kept1) at level level1; cut: an arc end even where nothing else changes.  An arc that is
// open ends at id when the run ends, turns round or is cut there, and one begins when the piece after is kept.
template <class Sink>
GPK_LC_FN void turn_to(Run& r, bool kept1, int level1, bool cut, End id, bool inside, P2 p, P2 q, int seg, int walk, Sink& out) {
    const bool was = r.open;
    const bool change = was != kept1 || (was && ((r.depth > 0) != (level1 > 0) || cut));
    if (change && was) turn_close(r, id, inside, p, q, arc_key(walk, seg, inside), out);
    r.depth = level1;
    if (!change) return;
    r.open = kept1;
    if (!kept1) return;
    if (r.stop) {  // second lap: no arc begins after the first break
        r.open = false;
        return;
    }
    out.begin_arc(with_far(id, p), q, arc_key(walk, seg, inside));
    out.coord(P2{id.x, id.y});
    r.emit = true;
}
// segment p -> q begins with a piece of class cls0; cut: p is a cut (is_cut_by of the piece before and cls0)
template <class Rule, class Sink>
GPK_LC_FN void turn_segment_begin(Run& r, int cls0, bool cut, P2 p, P2 q, int seg, int walk, int mode, Sink& out) {
    const bool kept0 = Rule::kept(cls0, walk, mode);
    if (!r.started) {
        r.started = true;
        r.head = r.open = kept0;
        r.emit = false;
        r.depth = level_of(cls0);
        return;
    }
    turn_to(r, kept0, level_of(cls0), cut, end_at_coord(p), false, p, q, seg, walk, out);
}
// the vertex `id` of the other row on the open segment, with the exact classes of the pieces before and after it
template <class Rule, class Sink>
GPK_LC_FN void turn_at_vertex(Run& r, int before, int after, End id, P2 p, P2 q, int seg, int walk, int mode, Sink& out) {
    turn_to(r, Rule::kept(after, walk, mode), level_of(after), is_cut_by<Rule>(before, after, walk, mode), id, true, p, q, seg, walk, out);
}
// a proper crossing into a piece of class `after`: the level moves, the run stays kept or dropped
template <class Sink>
GPK_LC_FN void turn_at_crossing(Run& r, int after, End id, P2 p, P2 q, int seg, int walk, Sink& out) {
    turn_to(r, r.open, r.depth + (after == CLS_INTERIOR ? 1 : -1), false, id, true, p, q, seg, walk, out);
}
template <class Sink>
GPK_LC_FN void turn_segment_end(Run& r, P2 p, P2 q, Sink& out) {
    if (r.open && r.emit) out.coord(q);
    r.prev_p = p;
}
// a run still open when the walk is back at the ring's first coordinate v0 (the start of segment seg0) ends there
template <class Sink>
GPK_LC_FN void turn_close_at_start(Run& r, P2 v0, int seg0, int walk, Sink& out) {
    if (r.open) turn_close(r, end_at_coord(v0), false, v0, v0, arc_key(walk, seg0, false), out);
}

// ---- junctions -------------------------------------------------------------------------------------------------------------------
// Where the ray J -> d lies when turning CLOCKWISE from the ray J -> r: 0: less than half a turn, 1: half a turn, 2: more, 3: a full
// turn (the same ray).  r, d != J.
template <class Orient>
GPK_LC_FN int cw_rank(P2 J, P2 r, P2 d, Orient orient) {
    const int s = orient(J, r, d);
    if (s < 0) return 0;
    if (s > 0) return 2;
    const bool same = r.x != J.x ? (r.x > J.x) == (d.x > J.x) : (r.y > J.y) == (d.y > J.y);
    return same ? 3 : 1;
}
// turning clockwise from J -> r, is J -> d1 met strictly before J -> d2
template <class Orient>
GPK_LC_FN bool cw_before(P2 J, P2 r, P2 d1, P2 d2, Orient orient) {
    const int k1 = cw_rank(J, r, d1, orient), k2 = cw_rank(J, r, d2, orient);
    if (k1 != k2) return k1 < k2;
    if (k1 == 1 || k1 == 3) return false;
    return orient(J, d1, d2) < 0;
}

// ---- rings -----------------------------------------------------------------------------------------------------------------------
// f(P2 v, bool computed) for every coordinate of the ring that starts at arc `first`, the closing one left out
template <class F>
GPK_LC_FN void ring_points(const Arc* arcs, const int* next, const P2* xy, int first, int n_arcs, F f) {
    int a = first;
    for (int it = 0; it < n_arcs; ++it) {
        const Arc& A = arcs[a];
        for (int j = 0; j + 1 < A.len; ++j) f(arc_coord(A, xy, j), j == 0 && A.s.ea >= 0);
        a = next[a];
        if (a == first) break;
    }
}

GPK_LC_FN bool lex_less(P2 u, P2 v) { return u.x < v.x || (u.x == v.x && u.y < v.y); }

// A coordinate of a ring with the EXACT directions in which the ring reaches and leaves it, as input coordinates: `in` lies on the
// carrier of the edge that arrives at v, behind v; `out` on the carrier of the edge that leaves it, ahead of v.  A computed crossing
// lies inside both carrying segments; it also gets their other ends: in_far ahead of v on the arriving carrier, out_far behind v on
// the leaving one.  The neighbouring COORDINATES are not used where one of the two is computed: a crossing is emitted within ulps of
// the end of its segment when it lies that close to it, and the direction between the two doubles is then noise.
struct Corner {
    P2 v;
    bool computed;
    P2 in, out, in_far, out_far;
};
// f(const Corner&) for every coordinate of the ring that starts at arc `first`, the closing one left out
template <class F>
GPK_LC_FN void ring_corners(const Arc* arcs, const int* next, const P2* xy, int first, int n_arcs, F f) {
    int prev = first;
    for (int it = 0; it < n_arcs && next[prev] != first; ++it) prev = next[prev];
    int a = first;
    for (int it = 0; it < n_arcs; ++it) {
        const Arc &A = arcs[a], &B = arcs[prev];
        for (int j = 0; j + 1 < A.len; ++j) {
            Corner c;
            c.v = arc_coord(A, xy, j);
            if (j == 0) {
                c.computed = A.s.ea >= 0;
                c.in = B.e_nb;
                c.out = A.s_nb;
                c.in_far = B.e.far;
                c.out_far = A.s.far;
            } else {
                c.computed = false;
                c.in = (j == 1 && A.s.ea >= 0) ? A.s.far : arc_coord(A, xy, j - 1);
                c.out = (j + 2 == A.len && A.e.ea >= 0) ? A.e.far : arc_coord(A, xy, j + 1);
                c.in_far = c.out_far = c.v;
            }
            f(c);
        }
        prev = a;
        a = next[a];
        if (a == first) break;
    }
}

// +1: counter-clockwise, -1: clockwise, 0: degenerate.  A corner is a local minimum of the lexicographic order when the ring reaches
// it from above and leaves it upwards: decided exactly, for an input coordinate by its two direction coordinates, for a crossing by
// the ends of its two carrying segments (the order is monotone along a segment).  M is the lowest of the local minima — of two
// coordinates ulps apart on one carrier exactly one is a local minimum, so the noise between them does not choose.  At an input
// coordinate M every incident edge leaves into the closed right half plane and the ring is counter-clockwise iff the lowest-lying of
// them is an outgoing one, whatever else touches M; the rays are the exact directions.  At a crossing M the ring turns from the
// carrier p1 -> q1 to the carrier p2 -> q2, and the turn is the side of q2 against p1 -> q1: exact, and independent of the rounded
// crossing.  Under the clip's and the union's rules no other ring passes through a crossing.  Under a rule with junctions at
// crossings (stitch<true>) a second ring does, in the OPPOSITE wedge of the two carriers: the corners handed over here are those of
// this ring alone (ring_corners follows its links), so the turn is that of this ring's own wedge and the other ring does not enter.
template <class Orient>
GPK_LC_FN int ring_sign(const Arc* arcs, const int* next, const P2* xy, int first, int n_arcs, Orient orient) {
    auto local_min = [](const Corner& c) {
        if (c.computed) return lex_less(c.in_far, c.in) && lex_less(c.out_far, c.out);  // (arriving downwards, leaving upwards)
        return lex_less(c.v, c.in) && lex_less(c.v, c.out);
    };
    P2 M{0.0, 0.0};
    int n = 0, have_m = 0;
    ring_corners(arcs, next, xy, first, n_arcs, [&](const Corner& c) {
        ++n;
        if (local_min(c) && (!have_m || lex_less(c.v, M))) {
            M = c.v;
            have_m = 1;
        }
    });
    if (n < 3 || !have_m) return 0;
    P2 low{0.0, 0.0};
    int low_out = 0, tie = 0, have = 0, turn = 0, at_input = 0;
    auto ray = [&](P2 d, int is_out) {
        const int s = have ? orient(M, low, d) : -1;  // < 0: d lies clockwise of (below) the lowest so far
        if (s < 0) {
            low = d;
            low_out = is_out;
            tie = 0;
            have = 1;
        } else if (s == 0 && is_out != low_out) {
            tie = 1;
        }
    };
    ring_corners(arcs, next, xy, first, n_arcs, [&](const Corner& c) {
        if (c.v.x != M.x || c.v.y != M.y || !local_min(c)) return;
        if (c.computed) {
            turn = orient(c.in, c.in_far, c.out);
        } else {
            at_input = 1;
            ray(c.in, 0);
            ray(c.out, 1);
        }
    });
    if (!at_input) return turn;
    if (!have || tie) return 0;
    return low_out ? 1 : -1;
}

// the exact position of t against the ring that starts at arc `first`: +1 inside, -1 outside, 0 on it
template <class Orient>
GPK_LC_FN int ring_position(const Arc* arcs, const int* next, const P2* xy, int first, int n_arcs, P2 t, Orient orient) {
    int inside = 0, on = 0, i = 0;
    P2 p0{0.0, 0.0}, u{0.0, 0.0};
    auto edge = [&](P2 a, P2 b) {
        if (t.x < fmin(a.x, b.x) || t.x > fmax(a.x, b.x) || t.y < fmin(a.y, b.y) || t.y > fmax(a.y, b.y)) {
            if ((a.y > t.y) == (b.y > t.y) || t.x > fmax(a.x, b.x)) return;
        }
        const int s = orient(a, b, t);
        if (s == 0) {
            if (t.x >= fmin(a.x, b.x) && t.x <= fmax(a.x, b.x) && t.y >= fmin(a.y, b.y) && t.y <= fmax(a.y, b.y)) on = 1;
            return;
        }
        if ((a.y > t.y) != (b.y > t.y) && (b.y > a.y) == (s > 0)) inside ^= 1;
    };
    ring_points(arcs, next, xy, first, n_arcs, [&](P2 v, bool) {
        if (i == 0) p0 = v; else edge(u, v);
        u = v;
        ++i;
    });
    if (i > 1) edge(u, p0);
    return on ? 0 : (inside ? 1 : -1);
}

// does the ring at `shell` enclose the ring at `hole` (rule 5)
template <class Orient>
GPK_LC_FN bool ring_encloses(const Arc* arcs, const int* next, const P2* xy, int shell, int hole, int n_arcs, Orient orient) {
    for (int pass = 0; pass < 2; ++pass) {  // input coordinates first, then computed crossings
        int verdict = 0;
        ring_points(arcs, next, xy, hole, n_arcs, [&](P2 v, bool computed) {
            if (verdict != 0 || computed != (pass == 1)) return;
            verdict = ring_position(arcs, next, xy, shell, n_arcs, v, orient);
        });
        if (verdict != 0) return verdict > 0;
    }
    return false;
}

GPK_LC_FN bool key_less(const Arc* arcs, int i, int j) { return arcs[i].key < arcs[j].key || (arcs[i].key == arcs[j].key && i < j); }

constexpr int ORDER_SHELL = 1 << 30;  // flag of an entry of the ring order: the ring opens a part

// The stitcher: the n arcs of a pair (coordinates in xy) into rings, signs and nesting.  Scratch: next, ring_first, order, info — n
// ints each.  On return next[i] is the arc after arc i in its ring and order[0 .. n_rings) lists the rings in output order, each as
// the number of its first arc, | ORDER_SHELL when the ring opens a part (the holes of a part follow its shell).  Returns ST_OK,
// ST_TOUCH, ST_EMPTY (n == 0) or ST_UNRESOLVED (the counts are then 0).  innermost (gpk_polyunion.h; left off by the two modes
// above): a hole goes to the enclosing shell that every other enclosing shell encloses, not to the first one in key order.
// CROSSINGS (gpk_polysymdiff.h; off for every rule under which at most one arc starts at a computed crossing): at a proper crossing
// two arcs end and two start, all four with one identity and one value, and the leftmost turn runs there as well — from the
// arriving carrier e_nb -> e.far the arc goes on along the one of the two halves of the other carrier whose end (s_nb) lies to the
// LEFT of it: one exact sign of four input coordinates, the computed value is not read.
template <bool CROSSINGS = false, class Orient>
GPK_LC_FN int stitch(const Arc* arcs, int n, const P2* xy, Orient orient, int* next, int* ring_first, int* order, int* info, int& n_parts,
                     int& n_rings, int& n_coords, bool innermost = false) {
    n_parts = n_rings = n_coords = 0;
    if (n == 0) return ST_EMPTY;
    bool junction = false;
    // links: the leftmost turn among the arcs that start where arc i ends; every arc must be chosen exactly once
    for (int i = 0; i < n; ++i) info[i] = 0;
    for (int i = 0; i < n; ++i) {
        const Arc& A = arcs[i];
        if (A.len < 2) return ST_UNRESOLVED;
        int best = -1;
        if (A.flags & ARC_WHOLE) {
            best = i;
        } else {
            for (int j = 0; j < n; ++j) {
                if ((arcs[j].flags & ARC_WHOLE) || !same_end(A.e, arcs[j].s)) continue;
                if (best < 0) {
                    best = j;
                    continue;
                }
                junction = true;
                if (A.e.ea < 0 && cw_before(P2{A.e.x, A.e.y}, A.e_nb, arcs[j].s_nb, arcs[best].s_nb, orient)) best = j;
                if constexpr (CROSSINGS) {
                    if (A.e.ea >= 0 && orient(A.e_nb, A.e.far, arcs[best].s_nb) <= 0 && orient(A.e_nb, A.e.far, arcs[j].s_nb) > 0) best = j;
                }
            }
        }
        if (best < 0) return ST_UNRESOLVED;
        next[i] = best;
        if (++info[best] > 1) return ST_UNRESOLVED;
    }
    // rings, each from its arc with the smallest key, in the order of those keys (info: 0 = not yet in a ring)
    for (int i = 0; i < n; ++i) info[i] = 0;
    int nr = 0, total = 0;
    for (int done = 0; done < n;) {
        int first = -1;
        for (int i = 0; i < n; ++i)
            if (!info[i] && (first < 0 || key_less(arcs, i, first))) first = i;
        int a = first, len = 1;
        for (int it = 0; it <= n; ++it) {
            if (info[a]) return ST_UNRESOLVED;  // (cannot happen: the links are a permutation)
            info[a] = nr + 1;
            ++done;
            len += arcs[a].len - 1;
            a = next[a];
            if (a == first) break;
        }
        if (a != first) return ST_UNRESOLVED;
        ring_first[nr++] = first;
        total += len;
    }
    // a ring that passes twice through one point touches itself there
    int status = ST_OK;
    if (junction)
        for (int i = 0; i < n && status == ST_OK; ++i)
            for (int j = i + 1; j < n; ++j)
                if (info[i] == info[j] && same_end(arcs[i].s, arcs[j].s)) {
                    status = ST_TOUCH;
                    break;
                }
    // signs (info[r]: +1 shell, -1 hole not yet placed, s + 2: hole of shell s), then nesting
    for (int r = 0; r < nr; ++r) {
        const int s = ring_sign(arcs, next, xy, ring_first[r], n, orient);
        if (s == 0) return ST_UNRESOLVED;
        info[r] = s;
    }
    for (int r = 0; r < nr; ++r) {
        if (info[r] != -1) continue;
        for (int s = 0; s < nr; ++s)
            if (info[s] == 1 && ring_encloses(arcs, next, xy, ring_first[s], ring_first[r], n, orient)) {
                // (innermost: a later shell that also encloses the hole takes it when the home so far encloses that shell)
                if (info[r] != -1 && !ring_encloses(arcs, next, xy, ring_first[info[r] - 2], ring_first[s], n, orient)) continue;
                info[r] = s + 2;
                if (!innermost) break;
            }
        if (info[r] == -1) return ST_UNRESOLVED;
    }
    int at = 0, parts = 0;
    for (int s = 0; s < nr; ++s) {
        if (info[s] != 1) continue;
        order[at++] = ring_first[s] | ORDER_SHELL;
        ++parts;
        for (int r = 0; r < nr; ++r)
            if (info[r] == s + 2) order[at++] = ring_first[r];
    }
    n_parts = parts;
    n_rings = nr;
    n_coords = total;
    return status;
}

}  // namespace pc
}  // namespace gpk

#if defined(__HIPCC__)
// ---- the device group routine -----------------------------------------------------------------------------------------------------
namespace gpk {
namespace pc {

// the edge of the usable row that carries the piece t -> w (t on it, the edge reaching beyond t towards w), as the number of its first
// coordinate; 0x7fffffff: none.  Rings of a valid row share no edge, so there is one.  Same value on every lane.
template <int G>
__device__ inline int carrying_edge(const DevGeo& P, int p0, int p1, double2 t, double2 w, int lane) {
    int best = 0x7fffffff;
    const bool by_x = w.x != t.x;
    const bool up = by_x ? w.x > t.x : w.y > t.y;
    for (int pt = p0; pt < p1; ++pt) {
        int r0, r1;
        if (!lp::part_of(P, pt, r0, r1)) continue;
        for (int r = r0; r < r1; ++r) {
            const int c0 = P.ring_off[r], m = P.ring_off[r + 1] - c0 - 1;
            for (int i = lane; i < m; i += G) {
                const double2 a = P.xy[c0 + i], b = P.xy[c0 + i + 1];
                if (cont::same_xy(a, b)) continue;
                if (t.x < fmin(a.x, b.x) || t.x > fmax(a.x, b.x) || t.y < fmin(a.y, b.y) || t.y > fmax(a.y, b.y)) continue;
                if (cont::orient(a, b, t) != 0 || cont::orient(a, b, w) != 0) continue;
                const double ta = by_x ? t.x : t.y, hi = by_x ? fmax(a.x, b.x) : fmax(a.y, b.y), lo = by_x ? fmin(a.x, b.x) : fmin(a.y, b.y);
                if (up ? hi > ta : lo < ta) best = best < c0 + i ? best : c0 + i;
            }
        }
    }
    return lp::group_imin<G>(best);
}

// the class of the piece t -> w next to t against the usable row P: lp::side_bits with BOUNDARY told apart by side
template <int G>
__device__ inline int piece_class(const DevGeo& P, int p0, int p1, double2 t, double2 w, int lane) {
    const int bits = lp::side_bits<G>(P, p0, p1, t, w, lane);
    if (bits != GPK_LP_BOUNDARY) return bits == GPK_LP_INTERIOR ? CLS_INTERIOR : CLS_EXTERIOR;
    const int e = carrying_edge<G>(P, p0, p1, t, w, lane);
    if (e == 0x7fffffff) return CLS_BOUNDARY_OPP;  // (cannot happen: BOUNDARY means along an edge)
    int ccw;
    bool hole;
    lc::ring_of<G>(P, p0, p1, e, lane, ccw, hole);
    return boundary_class(lc::p2(P.xy[e]), lc::p2(P.xy[e + 1]), lc::p2(t), lc::p2(w), ccw, hole);
}

// the lowest coordinate number in [c0, c1) of a vertex that lies where pq crosses ab properly (lp::vertex_at_crossing, with the
// vertex named); 0x7fffffff: none.  Same value on every lane.
template <int G>
__device__ inline int vertex_at_crossing_index(const double2* __restrict__ xy, int c0, int c1, double2 p, double2 q, double lx, double hx, double ly,
                                               double hy, double2 a, double2 b, int lane) {
    int best = 0x7fffffff;
    for (int i = c0 + lane; i < c1; i += G) {
        const double2 v = xy[i];
        if (v.x < lx || v.x > hx || v.y < ly || v.y > hy) continue;
        if (cont::orient(p, q, v) == 0 && cont::orient(a, b, v) == 0) best = best < i ? best : i;
    }
    return lp::group_imin<G>(best);
}

struct RowRef {
    int p0, p1;       // the row's members
    double4 box;      // the box of their shells
    int c0, c1;       // the row's coordinates
};

// One ring of the walked row W (coordinates [rc0, rc0 + n), a hole or not) against the usable row O.  walk: WALK_A when W is a.
template <int G, class Rule = ClipRule, class Sink>
__device__ inline void walk_ring_group(const DevGeo& W, const RowRef& w, int rc0, int n, bool is_hole, const DevGeo& O, const RowRef& other,
                                       const DevGeo& A, const DevGeo& B, int walk, int mode, P2 o, int lane, Sink& out) {
    cont::Ring R;
    (void)cont::ring_init<G>(R, W.xy + rc0, n, lane);
    const bool rev = is_hole ? R.ccw > 0 : R.ccw < 0;
    const int m = n - 1;
    const double4 box = other.box;
    const int max_events = 2 * (other.c1 - other.c0);
    Run run = run_start();
    const double2 v0 = W.xy[rev ? rc0 + m : rc0];
    double2 first_q = v0;
    int last_cls = 0;             // the class of the last piece of the segment before the current one
    int pp0 = 0, first_cls0 = 0;  // the position of the ring's first coordinate and the class of its first piece
    int seg0 = rc0 - w.c0;        // the number of the ring's first segment (read under a rule with directions by class only)
    (void)seg0;
    for (int lap = 0; lap < 2; ++lap) {
        if (lap == 1) {
            if (!run.head) {
                // the ring's first piece is not kept: a run still open ends at the first coordinate
                if constexpr (Rule::DIRECTION_BY_CLASS) {
                    turn_close_at_start(run, lc::p2(v0), seg0, walk, out);
                } else {
                    if (run.open && run.emit) out.end_arc(end_at_coord(lc::p2(v0)), run.prev_p, 0);
                }
                return;
            }
            if (!run.any_break) {
                // kept whole: one arc
                out.begin_arc(end_at_coord(lc::p2(v0)), lc::p2(first_q), (walk == WALK_B ? KEY_WALK_B : 0) | (2 * (rc0 - w.c0)));
                out.coord(lc::p2(v0));
                double2 p = v0;
                for (int k = 1; k <= m; ++k) {
                    const double2 q = W.xy[rev ? rc0 + m - k : rc0 + k];
                    if (cont::same_xy(p, q)) continue;
                    out.coord(lc::p2(q));
                    p = q;
                }
                // (a ring that merely touches the other row at its first coordinate is cut there: one arc, but not closed in itself)
                int whole = pp0 == GPK_LP_BOUNDARY && is_cut_by<Rule>(last_cls, first_cls0, walk, mode) ? 0 : ARC_WHOLE;
                if constexpr (Rule::DIRECTION_BY_CLASS) {
                    if (Rule::backwards(first_cls0, walk, mode)) whole |= ARC_BACKWARDS;  // (the key stays: the ring starts at v0 either way)
                }
                out.end_arc(end_at_coord(lc::p2(v0)), run.prev_p, whole);
                return;
            }
        }
        double2 p = v0;
        int pp = lp::coord_bits<G>(O, other.p0, other.p1, box, p, lane);
        bool seen = false;
        for (int k = 1; k <= m; ++k) {
            const int qi = rev ? rc0 + m - k : rc0 + k;
            const double2 q = W.xy[qi];
            if (cont::same_xy(p, q)) continue;
            if (!seen) first_q = q;
            seen = true;
            const int edge_w = rev ? qi : qi - 1;  // the segment as an edge of its column
            const int seg = (rc0 - w.c0) + k - 1;
            const int pq = lp::coord_bits<G>(O, other.p0, other.p1, box, q, lane);
            const int first = pp == GPK_LP_BOUNDARY ? piece_class<G>(O, other.p0, other.p1, p, q, lane) : (pp == GPK_LP_INTERIOR ? CLS_INTERIOR : CLS_EXTERIOR);
            const bool had = run.started;
            if (!had) {
                pp0 = pp;
                first_cls0 = first;
                seg0 = seg;
            }
            if constexpr (Rule::DIRECTION_BY_CLASS) {
                turn_segment_begin<Rule>(run, first, had && pp == GPK_LP_BOUNDARY && is_cut_by<Rule>(last_cls, first, walk, mode), lc::p2(p), lc::p2(q), seg, walk,
                                         mode, out);
            } else {
                run_segment_begin(run, Rule::kept(first, walk, mode), lc::p2(p), lc::p2(q), seg, walk, out);
                if (had && pp == GPK_LP_BOUNDARY && is_cut_by<Rule>(last_cls, first, walk, mode)) run_cut(run, end_at_coord(lc::p2(p)), false, lc::p2(p), lc::p2(q), seg, walk, out);
            }
            if (lap == 1 && !run.open) return;  // the head (or the run into it) has ended
            if (lap == 1) run.stop = true;      // from here on the first break ends the walk
            const double lx = fmin(p.x, q.x), hx = fmax(p.x, q.x), ly = fmin(p.y, q.y), hy = fmax(p.y, q.y);
            if (!(hx < box.x || lx > box.z || hy < box.y || ly > box.w)) {
                int cur = lc::NO_EVENT;
                for (int it = 0; it < max_events; ++it) {
                    cur = lc::next_event<G>(O, other.p0, other.p1, p, q, o, cur, lane);
                    if (cur == lc::NO_EVENT) break;
                    const lc::Event e = lc::event_of(cur, O.xy, lc::p2(p), lc::p2(q), o);
                    const double2 a = make_double2(e.a.x, e.a.y), b = make_double2(e.b.x, e.b.y);
                    if (e.kind == 0) {
                        const int after = piece_class<G>(O, other.p0, other.p1, a, q, lane), before = looking_back(piece_class<G>(O, other.p0, other.p1, a, p, lane));
                        if constexpr (Rule::DIRECTION_BY_CLASS) {
                            turn_at_vertex<Rule>(run, before, after, end_at_coord(e.a), lc::p2(p), lc::p2(q), seg, walk, mode, out);
                        } else {
                            const int type = (Rule::kept(after, walk, mode) ? 1 : 0) - (Rule::kept(before, walk, mode) ? 1 : 0);
                            if (type) run_transition(run, type, end_at_coord(e.a), lc::p2(p), lc::p2(q), seg, walk, out);
                            else if (is_cut_by<Rule>(before, after, walk, mode)) run_cut(run, end_at_coord(e.a), true, lc::p2(p), lc::p2(q), seg, walk, out);
                        }
                    } else if (!lp::vertex_at_crossing<G>(O.xy, other.c0, other.c1, p, q, lx, hx, ly, hy, a, b, lane)) {
                        int ccw;
                        bool hole;
                        lc::ring_of<G>(O, other.p0, other.p1, cur >> 1, lane, ccw, hole);
                        const int ea = walk == WALK_A ? edge_w : (cur >> 1), eb = walk == WALK_A ? (cur >> 1) : edge_w;
                        const bool a_left = walk == WALK_A ? !rev : (ccw > 0) != hole;
                        const P2 x = crossing_point(lc::p2(A.xy[ea]), lc::p2(A.xy[ea + 1]), lc::p2(B.xy[eb]), lc::p2(B.xy[eb + 1]), o, a_left, lc::DevOrient{});
                        // (a vertex of ANOTHER ring of the walked row at the crossing point — rings of a valid row may touch there — is what
                        // the other walk sees as a vertex on its open segment: the same identity and value here)
                        const int own = vertex_at_crossing_index<G>(W.xy, w.c0, w.c1, p, q, lx, hx, ly, hy, a, b, lane);
                        const End id = own != 0x7fffffff ? end_at_coord(lc::p2(W.xy[own])) : End{x.x, x.y, ea, eb, x};
                        if constexpr (Rule::DIRECTION_BY_CLASS) {
                            turn_at_crossing(run, class_after_crossing(cont::orient(a, b, q), ccw, hole), id, lc::p2(p), lc::p2(q), seg, walk, out);
                        } else {
                            run_transition(run, crossing_type_by<Rule>(cont::orient(a, b, q), ccw, hole, walk, mode), id, lc::p2(p), lc::p2(q), seg, walk, out);
                        }
                    }
                    if (lap == 1 && !run.open) return;
                }
            }
            if constexpr (Rule::DIRECTION_BY_CLASS) {
                turn_segment_end(run, lc::p2(p), lc::p2(q), out);
            } else {
                run_segment_end(run, lc::p2(p), lc::p2(q), out);
            }
            last_cls = pq == GPK_LP_BOUNDARY ? piece_class<G>(O, other.p0, other.p1, q, p, lane) : (pq == GPK_LP_INTERIOR ? CLS_INTERIOR : CLS_EXTERIOR);
            p = q;
            pp = pq;
        }
        if (!seen) return;  // (cannot happen: a ring that passes ring_init has distinct coordinates)
    }
    // (the second lap found no exit where the first had one: cannot happen, both make the same decisions; close what is open)
    if constexpr (Rule::DIRECTION_BY_CLASS) {
        turn_close_at_start(run, lc::p2(v0), seg0, walk, out);
    } else {
        if (run.open && run.emit) out.end_arc(end_at_coord(lc::p2(v0)), run.prev_p, 0);
    }
}

template <int G, class Rule = ClipRule, class Sink>
__device__ inline void walk_row_group(const DevGeo& W, const RowRef& w, const DevGeo& O, const RowRef& other, const DevGeo& A, const DevGeo& B,
                                      int walk, int mode, P2 o, int lane, Sink& out) {
    for (int pt = w.p0; pt < w.p1; ++pt) {
        int r0, r1;
        if (!lp::part_of(W, pt, r0, r1)) continue;
        for (int r = r0; r < r1; ++r) {
            const int c0 = W.ring_off[r], n = W.ring_off[r + 1] - c0;
            if (n == 0) continue;
            walk_ring_group<G, Rule>(W, w, c0, n, r > r0, O, other, A, B, walk, mode, o, lane, out);
        }
    }
}

template <int G>
__device__ inline bool row_ref(const DevGeo& P, int64_t i, int lane, RowRef& r) {
    if (i < 0 || !dev::row_ok(P, i)) return false;
    dev::geom_parts(P, i, r.p0, r.p1);
    if (!lp::polygon_row_ok<G>(P, r.p0, r.p1, lane, r.box)) return false;
    const int32_t* part_ring = P.type == GPK_GEOM_MULTIPOLYGON ? P.part_off : P.geom_off;
    r.c0 = P.ring_off[part_ring[r.p0]];
    r.c1 = P.ring_off[part_ring[r.p1]];
    return true;
}

// The arcs of clip(a[i], b[j]) into `out` (called with the same arguments on every lane of the group).  False: a null result row.
template <int G, class Rule = ClipRule, class Sink>
__device__ inline bool arcs_group(const DevGeo& a, int64_t i, const DevGeo& b, int64_t j, int mode, int lane, Sink& out) {
    RowRef ra, rb;
    if (!row_ref<G>(a, i, lane, ra) || !row_ref<G>(b, j, lane, rb)) return false;
    const P2 o = lc::local_origin(ra.box.x, ra.box.y, ra.box.z, ra.box.w, rb.box.x, rb.box.y, rb.box.z, rb.box.w);
    walk_row_group<G, Rule>(a, ra, b, rb, a, b, WALK_A, mode, o, lane, out);
    walk_row_group<G, Rule>(b, rb, a, ra, a, b, WALK_B, mode, o, lane, out);
    return true;
}

}  // namespace pc
}  // namespace gpk
#endif
