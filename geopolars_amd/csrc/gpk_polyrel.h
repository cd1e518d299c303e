// gpk_polyrel.h — how two polygonal geometries lie to each other: the 4-bit mask of gpk_polygon_relation (include/geopolars_hip.h).
// A, B = POLYGON / MULTIPOLYGON rows, closed regular sets (A = closure of int A); int and ext are open.  GPK_PP_INTERIORS: int A and
// int B share a point, GPK_PP_BOUNDARIES: a ring of A and a ring of B share a point, GPK_PP_A_OUTSIDE: int A has a point in ext B,
// GPK_PP_B_OUTSIDE: int B has a point in ext A.  Every named area / area predicate is a function of the mask.
//
//   m_ab = the line x polygon mask (gpk_linearea.h) of the rings of A, taken as closed coordinate sequences, against B:
//          a ring of A has a point in int B (1), on a ring of B (2), in ext B (4);         m_ba = the same with the roles swapped
//   BOUNDARIES = m_ab & 2
//   INTERIORS  = (m_ab & 1) | (m_ba & 1) | same_side
//   A_OUTSIDE  = (m_ab & 4) | (m_ba & 1) | opposite_side
//   B_OUTSIDE  = (m_ba & 4) | (m_ab & 1) | opposite_side
// same_side / opposite_side: an edge of A and an edge of B are collinear and overlap in a piece of positive length (two exact
// orientations and coordinate comparisons), and the two interiors lie on the same hand of that piece, or on opposite hands.  The
// interior hand of an edge: the left of a counter-clockwise shell or a clockwise hole, else the right (the ring's orientation is
// cont::ring_init's turn at the smallest vertex).
//
// Why the bits that are set are right.  A point x of a ring of A in ext B: every neighbourhood of x holds points of int A (A is the
// closure of its interior), and a small one lies in ext B (open) — A_OUTSIDE.  A point x of a ring of B in int A: every neighbourhood
// holds points of int B and points of ext B (the boundary of a closed regular set is the boundary of its exterior too), a small one
// lies in int A — INTERIORS and A_OUTSIDE.  At an inner point of an overlap piece, away from the finitely many vertices, each
// geometry is locally a half-plane bounded by the piece (an edge of a valid geometry carries no second ring of the same geometry):
// on the same hand the interiors share points, on opposite hands each interior lies in the other's exterior.
// Why nothing is missed.  Let C be a component of int A ∩ ext B (for A_OUTSIDE; int A ∩ int B for INTERIORS, int B ∩ ext A for
// B_OUTSIDE).  Its boundary has positive length and lies on rings of A and of B; take a point y of it that is no vertex and no
// crossing point of either geometry.  If y is on a ring of A only, it is in cl(ext B) minus the rings of B = ext B: m_ab & 4.  If it
// is on a ring of B only, it is in int A: m_ba & 1.  If it is on both, the two rings run along each other there — an overlap piece,
// with int A on C's hand and int B on the other: opposite_side.  The same three cases give INTERIORS (m_ab & 1, m_ba & 1, same_side).
// So a component whose boundary never enters the other geometry's interior or exterior shows up as an overlap piece: equal polygons
// (3), a polygon that fills a hole of the other exactly (14), {A1 = B1, A2 = the filling of B2's hole} (15, through the side rule alone).
// Rings of one geometry that touch at single points (hole-shell, hole-hole, part-part) while the other geometry passes through the
// point: the walk judges every piece next to a touch point against all rings of all parts (the ring-touch rule of gpk_linearea.h), and
// the argument above only uses generic boundary points, so such points need no rule of their own here.
//
// G lanes work on one (A, B) pair exactly as in gpk_linearea.h: the edges of the geometry walked against are strided over the lanes,
// every branch around a reduction is group-uniform.  When the first walk finds no shared boundary point, every ring of B lies in
// int A or in ext A as a whole and one coordinate per ring replaces the second walk; the overlap pass runs only when BOUNDARIES is
// set and a bit it could add is still missing.  Cost per pair: 2 x (coordinates of one) x (edges of the other) position tests, the
// same number of box-pruned event tests, one pass over the other geometry per touch event, and edges x edges box tests with two
// orientations where boxes meet for the overlap pass.  Pairs whose shell boxes are apart cost the two validity passes.
//
// Rows: a null row, one without a non-empty member, or one with a ring that fails cont::ring_init: 0, on either side.  Empty members
// are ignored.  Invalid polygons: the mask is unspecified, the routine terminates.
#pragma once

#include "gpk_linearea.h"

namespace gpk {
namespace pp {

constexpr int PP_ALL = GPK_PP_INTERIORS | GPK_PP_BOUNDARIES | GPK_PP_A_OUTSIDE | GPK_PP_B_OUTSIDE;

// When a caller needs less than the mask: stop as soon as one of `any` is set or all of `all` are.  {0, PP_ALL}: the full mask.
struct Stop {
    int any, all;
};
__device__ __forceinline__ bool done(int mask, Stop st) { return (mask & st.any) != 0 || (mask & st.all) == st.all; }

// the predicate ids of gpk_polygon_relation_join over the mask
__host__ __device__ inline bool predicate_of(int mask, int pred) {
    switch (pred) {
    case GPK_PP_PRED_INTERSECTS: return (mask & (GPK_PP_INTERIORS | GPK_PP_BOUNDARIES)) != 0;
    case GPK_PP_PRED_WITHIN: return (mask & GPK_PP_INTERIORS) && !(mask & GPK_PP_A_OUTSIDE);
    case GPK_PP_PRED_CONTAINS: return (mask & GPK_PP_INTERIORS) && !(mask & GPK_PP_B_OUTSIDE);
    case GPK_PP_PRED_TOUCHES: return (mask & GPK_PP_BOUNDARIES) && !(mask & GPK_PP_INTERIORS);
    case GPK_PP_PRED_OVERLAPS: return (mask & 13) == 13;
    case GPK_PP_PRED_EQUALS: return (mask & GPK_PP_INTERIORS) && !(mask & (GPK_PP_A_OUTSIDE | GPK_PP_B_OUTSIDE));
    case GPK_PP_PRED_CONTAINS_PROPERLY: return (mask & 11) == GPK_PP_INTERIORS;
    default: return false;
    }
}
// the bits that settle a predicate before the mask is complete (touches fails at the first INTERIORS bit, ...)
inline Stop stop_of(int pred) {
    switch (pred) {
    case GPK_PP_PRED_INTERSECTS: return Stop{GPK_PP_INTERIORS | GPK_PP_BOUNDARIES, PP_ALL};
    case GPK_PP_PRED_WITHIN: return Stop{GPK_PP_A_OUTSIDE, PP_ALL};
    case GPK_PP_PRED_CONTAINS: return Stop{GPK_PP_B_OUTSIDE, PP_ALL};
    case GPK_PP_PRED_TOUCHES: return Stop{GPK_PP_INTERIORS, PP_ALL};
    case GPK_PP_PRED_OVERLAPS: return Stop{0, 13};
    case GPK_PP_PRED_EQUALS: return Stop{GPK_PP_A_OUTSIDE | GPK_PP_B_OUTSIDE, PP_ALL};
    case GPK_PP_PRED_CONTAINS_PROPERLY: return Stop{GPK_PP_BOUNDARIES | GPK_PP_B_OUTSIDE, PP_ALL};
    default: return Stop{0, PP_ALL};
    }
}

// what the walk of A's rings against B (m_ab), and of B's rings against A (m_ba), says about the pair
__device__ __forceinline__ int bits_of_ab(int m) {
    return (m & GPK_LP_INTERIOR ? GPK_PP_INTERIORS | GPK_PP_B_OUTSIDE : 0) | (m & GPK_LP_BOUNDARY ? GPK_PP_BOUNDARIES : 0) |
           (m & GPK_LP_EXTERIOR ? GPK_PP_A_OUTSIDE : 0);
}
__device__ __forceinline__ int bits_of_ba(int m) {
    return (m & GPK_LP_INTERIOR ? GPK_PP_INTERIORS | GPK_PP_A_OUTSIDE : 0) | (m & GPK_LP_BOUNDARY ? GPK_PP_BOUNDARIES : 0) |
           (m & GPK_LP_EXTERIOR ? GPK_PP_B_OUTSIDE : 0);
}

__device__ __forceinline__ RowSeqs ring_seqs(const DevGeo& P, int64_t i) {
    return P.type == GPK_GEOM_POLYGON ? row_seqs<GPK_GEOM_POLYGON>(P, i) : row_seqs<GPK_GEOM_MULTIPOLYGON>(P, i);
}

// The overlap pieces of the two usable rows: GPK_PP_INTERIORS for a piece with both interiors on the same hand, GPK_PP_A_OUTSIDE |
// GPK_PP_B_OUTSIDE for one with the interiors on opposite hands.  Ends once all bits of `want` are found.
template <int G>
__device__ inline int overlap_bits(const DevGeo& A, int a0, int a1, const DevGeo& B, int b0, int b1, double4 box_b, int lane, int want) {
    constexpr int OPPOSITE = GPK_PP_A_OUTSIDE | GPK_PP_B_OUTSIDE;
    int bits = 0;
    for (int pa = a0; pa < a1; ++pa) {
        int ar0, ar1;
        if (!lp::part_of(A, pa, ar0, ar1)) continue;
        for (int ra = ar0; ra < ar1; ++ra) {
            const int ac0 = A.ring_off[ra], an = A.ring_off[ra + 1] - ac0;
            if (an == 0) continue;
            cont::Ring RA;
            (void)cont::ring_init<G>(RA, A.xy + ac0, an, lane);
            const bool a_left = (RA.ccw > 0) != (ra > ar0);  // int A on the left of the ring's edges
            for (int pb = b0; pb < b1; ++pb) {
                int br0, br1;
                if (!lp::part_of(B, pb, br0, br1)) continue;
                for (int rb = br0; rb < br1; ++rb) {
                    const int bc0 = B.ring_off[rb], bn = B.ring_off[rb + 1] - bc0;
                    if (bn == 0) continue;
                    cont::Ring RB;
                    (void)cont::ring_init<G>(RB, B.xy + bc0, bn, lane);
                    const bool b_left = (RB.ccw > 0) != (rb > br0);
                    int found = 0;
                    for (int i = 0; i < RA.m; ++i) {
                        const double2 a = RA.v[i], b = RA.v[i + 1];
                        if (cont::same_xy(a, b)) continue;
                        const double lx = fmin(a.x, b.x), hx = fmax(a.x, b.x), ly = fmin(a.y, b.y), hy = fmax(a.y, b.y);
                        if (hx < box_b.x || lx > box_b.z || hy < box_b.y || ly > box_b.w) continue;
                        const bool by_x = a.x != b.x;  // the axis on which the line through a and b is not constant
                        const double a_lo = by_x ? lx : ly, a_hi = by_x ? hx : hy;
                        const bool a_up = by_x ? b.x > a.x : b.y > a.y;
                        for (int j = lane; j < RB.m; j += G) {
                            const double2 c = RB.v[j], d = RB.v[j + 1];
                            if (fmax(c.x, d.x) < lx || fmin(c.x, d.x) > hx || fmax(c.y, d.y) < ly || fmin(c.y, d.y) > hy) continue;
                            if (cont::same_xy(c, d) || cont::orient(a, b, c) != 0 || cont::orient(a, b, d) != 0) continue;
                            const double c1 = by_x ? c.x : c.y, d1 = by_x ? d.x : d.y;
                            if (!(fmax(a_lo, fmin(c1, d1)) < fmin(a_hi, fmax(c1, d1)))) continue;  // they share a point at most
                            const bool same_way = a_up == (d1 > c1);
                            found |= (a_left == b_left) == same_way ? GPK_PP_INTERIORS : OPPOSITE;
                        }
                    }
                    bits |= dev::group_or<G>(found);
                    if ((bits & want) == want) return bits;
                }
            }
        }
    }
    return bits;
}

// The mask of row i of `a` against row j of `b` (both POLYGON | MULTIPOLYGON); rows out of range behave like null rows.  With `st`
// the work ends as soon as the bits a caller needs are settled (the mask is then partial).  Same value on every lane of the group.
template <int G>
__device__ inline int polygon_polygon_mask_group(const DevGeo& a, int64_t i, const DevGeo& b, int64_t j, int lane, Stop st = Stop{0, PP_ALL}) {
    if (!dev::row_ok(a, i) || !dev::row_ok(b, j)) return 0;
    int a0, a1, b0, b1;
    dev::geom_parts(a, i, a0, a1);
    dev::geom_parts(b, j, b0, b1);
    double4 box_a, box_b;
    if (!lp::polygon_row_ok<G>(a, a0, a1, lane, box_a) || !lp::polygon_row_ok<G>(b, b0, b1, lane, box_b)) return 0;
    if (box_a.z < box_b.x || box_a.x > box_b.z || box_a.w < box_b.y || box_a.y > box_b.w) return GPK_PP_A_OUTSIDE | GPK_PP_B_OUTSIDE;
    const RowSeqs sa = ring_seqs(a, i), sb = ring_seqs(b, j);

    int mask = bits_of_ab(lp::sequences_mask_group<G>(sa, b, b0, b1, box_b, lane, [st](int m) { return done(bits_of_ab(m), st); }));
    if (done(mask, st)) return mask;
    if (mask & GPK_PP_BOUNDARIES) {
        const int seen = mask;
        mask |= bits_of_ba(lp::sequences_mask_group<G>(sb, a, a0, a1, box_a, lane, [st, seen](int m) { return done(seen | bits_of_ba(m), st); }));
    } else {
        // no ring of B meets a ring of A: a ring of B lies where its first coordinate lies
        for (int s = sb.s0; s < sb.s1 && !done(mask, st); ++s) {
            const int c0 = sb.so[s];
            if (sb.so[s + 1] > c0) mask |= bits_of_ba(lp::coord_bits<G>(a, a0, a1, box_a, sb.xy[c0], lane));
        }
    }
    if (done(mask, st) || !(mask & GPK_PP_BOUNDARIES)) return mask;
    const int want = ~mask & (GPK_PP_INTERIORS | GPK_PP_A_OUTSIDE | GPK_PP_B_OUTSIDE);
    if (want) mask |= overlap_bits<G>(a, a0, a1, b, b0, b1, box_b, lane, want);
    return mask;
}

// lanes per pair, lp::relation_group_size's rule: the lanes stride the ring edges of either column in turn, so the larger of the two
// mean coordinate counts decides
static inline int relation_group_size(const DevGeo& a, const DevGeo& b) {
    const int ga = lp::relation_group_size(a, a), gb = lp::relation_group_size(b, b);
    return ga > gb ? ga : gb;
}

}  // namespace pp
}  // namespace gpk
