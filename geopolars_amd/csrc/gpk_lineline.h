// gpk_lineline.h — how two lineal geometries lie to each other: the 7-bit mask of gpk_line_relation (include/geopolars_hip.h).
// A, B = LINESTRING / MULTILINESTRING rows, each the closed point set of its segments and coordinates.  The boundary of a row follows
// the mod-2 rule: every non-empty member counts its first and its last coordinate once each, a point counted an odd number of times
// is a boundary point, every other point of the row is interior.  Nothing assumes a row is simple.
//
// A point shared by A and B is (a) a coordinate of one row that lies on the other, (b) the one point of a proper crossing of two
// segments, or (c) an inner point of a piece two collinear segments share: two non-degenerate segments meet in nothing, one point
// or a piece (val::seg_meet), the one point is inside both or a coordinate of one, and the two ends of a piece are coordinates.
// Members of one coordinate and zero-length segments are coordinates only.  So the mask is the OR of
//   coordinates   every coordinate c of A on B sets the bit named by (status of c in A, status of c in B), one not on B sets
//                 A_OUTSIDE; the same for the coordinates of B.  The status of a point x in a row is the parity of the member ends
//                 equal to x (ends_at), counted ON THE FLY: there is no pre-pass and no table of boundary points.
//   crossings     a proper crossing sets the bit named by (parity of A's member ends at the crossing, the same of B): the point need
//                 not be representable, but a coordinate v sits there exactly when it lies in both segments' boxes and
//                 orient(a, b, v) == 0 && orient(c, d, v) == 0 (the lines through ab and cd meet in that point only).
//   pieces        seg_meet == 2 sets INTERIORS | SHARED_PIECE (a piece holds infinitely many points and finitely many of them are
//                 boundary points of either row).
//   covering      when every coordinate of A is on B: a non-degenerate segment of A lies in B exactly when the pieces it shares
//                 with B's collinear segments cover it (the other segments of B meet it in finitely many points, and B is closed).
//                 A frontier runs from the segment's lower end along the axis on which it is not constant: every lane moves it over
//                 its own share of B's segments, the group takes the maximum, until the upper end is reached or a round moves
//                 nothing — then a point of A is no point of B.  All comparisons are between coordinates of collinear points.
//
// G lanes work on one pair.  The coordinate or segment of the walked row is the same on all lanes, the other row's coordinates are
// strided over the lanes, every reduction sits in group-uniform control flow.  Segments of a row whose box misses the other row's box
// take part in no segment test, coordinates outside it are off the other row at once.  Cost per pair with n, m coordinates and boxes
// that meet: n m / G box tests for the segment pass (four orientations where boxes meet), 2 n m / G point-in-box tests for the two
// coordinate passes (one orientation where a point is in a segment's box), and for rows that lie in each other the covering rounds.
// A crossing or an on-coordinate costs one pass over the members' ends of both rows on the lane that found it.
//
// Rows: null, without a coordinate, or with a NaN or infinite coordinate: 0.  Empty members are ignored.
#pragma once

#include "gpk_contains.h"
#include "gpk_device.h"
#include "gpk_linearea.h"
#include "gpk_pairdist.h"
#include "gpk_validity.h"

namespace gpk {
namespace ll {

constexpr int LL_ALL = GPK_LL_INTERIORS | GPK_LL_SHARED_PIECE | GPK_LL_INT_BND | GPK_LL_BND_INT | GPK_LL_BND_BND | GPK_LL_A_OUTSIDE | GPK_LL_B_OUTSIDE;
constexpr int LL_SHARED = GPK_LL_INTERIORS | GPK_LL_SHARED_PIECE | GPK_LL_INT_BND | GPK_LL_BND_INT | GPK_LL_BND_BND;

// When a caller needs less than the mask: stop as soon as one of `any` is set or all of `all` are.  {0, LL_ALL}: the full mask.
struct Stop {
    int any, all;
};
__device__ __forceinline__ bool done(int mask, Stop st) { return (mask & st.any) != 0 || (mask & st.all) == st.all; }

// the predicate ids of gpk_line_relation_join over the mask
__host__ __device__ inline bool predicate_of(int mask, int pred) {
    switch (pred) {
    case GPK_LL_PRED_INTERSECTS: return (mask & LL_SHARED) != 0;
    case GPK_LL_PRED_WITHIN: return (mask & GPK_LL_INTERIORS) && !(mask & GPK_LL_A_OUTSIDE);
    case GPK_LL_PRED_CONTAINS: return (mask & GPK_LL_INTERIORS) && !(mask & GPK_LL_B_OUTSIDE);
    case GPK_LL_PRED_COVERED_BY: return (mask & LL_SHARED) && !(mask & GPK_LL_A_OUTSIDE);
    case GPK_LL_PRED_COVERS: return (mask & LL_SHARED) && !(mask & GPK_LL_B_OUTSIDE);
    case GPK_LL_PRED_CROSSES: return (mask & GPK_LL_INTERIORS) && !(mask & GPK_LL_SHARED_PIECE);
    case GPK_LL_PRED_TOUCHES: return (mask & (GPK_LL_INT_BND | GPK_LL_BND_INT | GPK_LL_BND_BND)) && !(mask & GPK_LL_INTERIORS);
    case GPK_LL_PRED_OVERLAPS: return (mask & GPK_LL_SHARED_PIECE) && (mask & GPK_LL_A_OUTSIDE) && (mask & GPK_LL_B_OUTSIDE);
    case GPK_LL_PRED_EQUALS: return (mask & GPK_LL_INTERIORS) && !(mask & (GPK_LL_A_OUTSIDE | GPK_LL_B_OUTSIDE));
    default: return false;
    }
}
// the bits that settle a predicate before the mask is complete (touches fails at the first INTERIORS bit, ...)
inline Stop stop_of(int pred) {
    switch (pred) {
    case GPK_LL_PRED_INTERSECTS: return Stop{LL_SHARED, LL_ALL};
    case GPK_LL_PRED_WITHIN:
    case GPK_LL_PRED_COVERED_BY: return Stop{GPK_LL_A_OUTSIDE, LL_ALL};
    case GPK_LL_PRED_CONTAINS:
    case GPK_LL_PRED_COVERS: return Stop{GPK_LL_B_OUTSIDE, LL_ALL};
    case GPK_LL_PRED_CROSSES: return Stop{GPK_LL_SHARED_PIECE, LL_ALL};
    case GPK_LL_PRED_TOUCHES: return Stop{GPK_LL_INTERIORS, LL_ALL};
    case GPK_LL_PRED_OVERLAPS: return Stop{0, GPK_LL_SHARED_PIECE | GPK_LL_A_OUTSIDE | GPK_LL_B_OUTSIDE};
    case GPK_LL_PRED_EQUALS: return Stop{GPK_LL_A_OUTSIDE | GPK_LL_B_OUTSIDE, LL_ALL};
    default: return Stop{0, LL_ALL};
    }
}

// the bit of a shared point from its status in A and in B (true: a boundary point)
__device__ __forceinline__ int shared_bit(bool bnd_a, bool bnd_b) {
    return bnd_a ? (bnd_b ? GPK_LL_BND_BND : GPK_LL_BND_INT) : (bnd_b ? GPK_LL_INT_BND : GPK_LL_INTERIORS);
}

// how many member ends of the row are the point x (first and last coordinate of every non-empty member, once each): odd — x is a
// boundary point of the row.  One lane, no reduction: it is called from divergent code.
__device__ inline int ends_at(const RowSeqs& r, double2 x) {
    int n = 0;
    for (int s = r.s0; s < r.s1; ++s) {
        const int c0 = r.so[s], c1 = r.so[s + 1];
        if (c1 <= c0) continue;
        n += (cont::same_xy(r.xy[c0], x) ? 1 : 0) + (cont::same_xy(r.xy[c1 - 1], x) ? 1 : 0);
    }
    return n;
}
// the same for the point where ab and cd cross properly; [lx, hx] x [ly, hy]: the intersection of the two segments' boxes
__device__ inline int ends_at_crossing(const RowSeqs& r, double2 a, double2 b, double2 c, double2 d, double lx, double hx, double ly, double hy) {
    int n = 0;
    for (int s = r.s0; s < r.s1; ++s) {
        const int c0 = r.so[s], c1 = r.so[s + 1];
        if (c1 <= c0) continue;
        for (int e = 0; e < 2; ++e) {
            const double2 v = r.xy[e ? c1 - 1 : c0];
            if (v.x < lx || v.x > hx || v.y < ly || v.y > hy) continue;
            if (cont::orient(a, b, v) == 0 && cont::orient(c, d, v) == 0) ++n;
        }
    }
    return n;
}

// is coordinate j of the row the start of a segment (not the last coordinate of its member)
__device__ __forceinline__ bool starts_segment(const RowSeqs& r, int j) { return j + 1 < r.so[seq_of(r.so, r.s0, r.s1, j) + 1]; }

// the row's coordinates are finite (else false), and their box
template <int G>
__device__ inline bool row_box(const RowSeqs& r, int lane, double4& box) {
    double lx = INFINITY, ly = INFINITY, hx = -INFINITY, hy = -INFINITY;
    int bad = 0;
    for (int c = r.c0 + lane; c < r.c1; c += G) {
        const double2 v = r.xy[c];
        bad |= val::finite2(v) ? 0 : 1;
        lx = fmin(lx, v.x);
        ly = fmin(ly, v.y);
        hx = fmax(hx, v.x);
        hy = fmax(hy, v.y);
    }
    if (dev::group_or<G>(bad)) return false;
    box = make_double4(dev::group_min<G>(lx), dev::group_min<G>(ly), dev::group_max<G>(hx), dev::group_max<G>(hy));
    return true;
}

// does the point p lie on the row `o`: on one of its coordinates or inside one of its segments
template <int G>
__device__ inline bool on_row(const RowSeqs& o, double2 p, int lane) {
    int on = 0;
    for (int j = o.c0 + lane; j < o.c1 && !on; j += G) {
        const double2 c = o.xy[j];
        if (cont::same_xy(c, p)) {
            on = 1;
        } else if (j + 1 < o.c1) {
            const double2 d = o.xy[j + 1];
            if (p.x < fmin(c.x, d.x) || p.x > fmax(c.x, d.x) || p.y < fmin(c.y, d.y) || p.y > fmax(c.y, d.y)) continue;
            if (cont::orient(c, d, p) == 0 && starts_segment(o, j)) on = 1;
        }
    }
    return dev::group_or<G>(on) != 0;
}

// The coordinates of the row `w` against the row `o` with the box `obox`: the shared-point bits, `w_first` says whether w is A (the
// bits name A's status first), and `outside` (A_OUTSIDE for w = A) for a coordinate that is no point of `o`.
template <int G>
__device__ inline int coordinate_bits(const RowSeqs& w, const RowSeqs& o, double4 obox, bool w_first, int outside, int lane, int seen, Stop st) {
    int mask = 0;
    for (int c = w.c0; c < w.c1; ++c) {
        const double2 p = w.xy[c];
        if (c > w.c0 && cont::same_xy(p, w.xy[c - 1])) continue;  // (decided with the coordinate before it)
        if (p.x < obox.x || p.x > obox.z || p.y < obox.y || p.y > obox.w || !on_row<G>(o, p, lane)) {
            mask |= outside;
        } else {
            const bool bw = ends_at(w, p) & 1, bo = ends_at(o, p) & 1;
            mask |= w_first ? shared_bit(bw, bo) : shared_bit(bo, bw);
        }
        if (done(seen | mask, st)) break;
    }
    return mask;
}

// The segments of A against the segments of B: proper crossings and shared pieces.
template <int G>
__device__ inline int segment_bits(const RowSeqs& A, const RowSeqs& B, double4 box_b, int lane, int seen, Stop st) {
    int mask = 0;
    for (int s = A.s0; s < A.s1; ++s) {
        const int i0 = A.so[s], i1 = A.so[s + 1];
        for (int i = i0; i + 1 < i1; ++i) {
            const double2 a = A.xy[i], b = A.xy[i + 1];
            if (cont::same_xy(a, b)) continue;
            const double lx = fmin(a.x, b.x), hx = fmax(a.x, b.x), ly = fmin(a.y, b.y), hy = fmax(a.y, b.y);
            if (hx < box_b.x || lx > box_b.z || hy < box_b.y || ly > box_b.w) continue;
            int found = 0;
            for (int j = B.c0 + lane; j + 1 < B.c1; j += G) {
                const double2 c = B.xy[j], d = B.xy[j + 1];
                const double clx = fmin(c.x, d.x), chx = fmax(c.x, d.x), cly = fmin(c.y, d.y), chy = fmax(c.y, d.y);
                if (chx < lx || clx > hx || chy < ly || cly > hy) continue;
                if (cont::same_xy(c, d) || !starts_segment(B, j)) continue;
                double2 x;
                bool proper;
                const int m = val::seg_meet(a, b, c, d, x, proper);
                if (m == 2) {
                    found |= GPK_LL_INTERIORS | GPK_LL_SHARED_PIECE;
                } else if (m == 1 && proper) {
                    const double ix0 = fmax(lx, clx), ix1 = fmin(hx, chx), iy0 = fmax(ly, cly), iy1 = fmin(hy, chy);
                    found |= shared_bit(ends_at_crossing(A, a, b, c, d, ix0, ix1, iy0, iy1) & 1, ends_at_crossing(B, a, b, c, d, ix0, ix1, iy0, iy1) & 1);
                }  // (one point that is a coordinate: the coordinate passes see it)
            }
            mask |= dev::group_or<G>(found);
            if (done(seen | mask, st)) return mask;
        }
    }
    return mask;
}

// does the row `o` cover the segment ab (a != b) of the other row
template <int G>
__device__ inline bool segment_covered(double2 a, double2 b, const RowSeqs& o, int lane) {
    const bool by_x = a.x != b.x;  // the axis on which the line through a and b is not constant
    const double lx = fmin(a.x, b.x), hx = fmax(a.x, b.x), ly = fmin(a.y, b.y), hy = fmax(a.y, b.y);
    const double hi = by_x ? hx : hy;
    double f = by_x ? lx : ly;  // [the lower end, f] is covered
    while (f < hi) {
        double fl = f;
        for (int j = o.c0 + lane; j + 1 < o.c1; j += G) {
            const double2 c = o.xy[j], d = o.xy[j + 1];
            if (fmax(c.x, d.x) < lx || fmin(c.x, d.x) > hx || fmax(c.y, d.y) < ly || fmin(c.y, d.y) > hy) continue;
            const double c1 = by_x ? c.x : c.y, d1 = by_x ? d.x : d.y;
            const double p_lo = fmin(c1, d1), p_hi = fmax(c1, d1);
            if (p_lo > fl || !(p_hi > fl)) continue;
            if (cont::orient(a, b, c) != 0 || cont::orient(a, b, d) != 0 || !starts_segment(o, j)) continue;
            fl = p_hi;
        }
        fl = dev::group_max<G>(fl);
        if (!(fl > f)) return false;
        f = fl;
    }
    return true;
}

// every non-degenerate segment of `w`, all of whose coordinates lie on `o`, is covered by `o`
template <int G>
__device__ inline bool row_covered(const RowSeqs& w, const RowSeqs& o, int lane) {
    for (int s = w.s0; s < w.s1; ++s) {
        const int i0 = w.so[s], i1 = w.so[s + 1];
        for (int i = i0; i + 1 < i1; ++i) {
            const double2 a = w.xy[i], b = w.xy[i + 1];
            if (!cont::same_xy(a, b) && !segment_covered<G>(a, b, o, lane)) return false;
        }
    }
    return true;
}

// The mask of row i of `a` against row j of `b` (both LINESTRING | MULTILINESTRING); rows out of range behave like null rows.  With
// `st` the work ends as soon as the bits a caller needs are settled (the mask is then partial).  Same value on every lane of the group.
template <int G>
__device__ inline int line_line_mask_group(const DevGeo& a, int64_t i, const DevGeo& b, int64_t j, int lane, Stop st = Stop{0, LL_ALL}) {
    if (!dev::row_ok(a, i) || !dev::row_ok(b, j)) return 0;
    const RowSeqs A = lp::line_seqs(a, i), B = lp::line_seqs(b, j);
    if (A.c1 <= A.c0 || B.c1 <= B.c0) return 0;
    double4 box_a, box_b;
    if (!row_box<G>(A, lane, box_a) || !row_box<G>(B, lane, box_b)) return 0;
    if (box_a.z < box_b.x || box_a.x > box_b.z || box_a.w < box_b.y || box_a.y > box_b.w) return GPK_LL_A_OUTSIDE | GPK_LL_B_OUTSIDE;

    int mask = segment_bits<G>(A, B, box_b, lane, 0, st);
    if (done(mask, st)) return mask;
    mask |= coordinate_bits<G>(A, B, box_b, true, GPK_LL_A_OUTSIDE, lane, mask, st);
    if (done(mask, st)) return mask;
    mask |= coordinate_bits<G>(B, A, box_a, false, GPK_LL_B_OUTSIDE, lane, mask, st);
    if (done(mask, st)) return mask;
    if (!(mask & GPK_LL_A_OUTSIDE) && !row_covered<G>(A, B, lane)) mask |= GPK_LL_A_OUTSIDE;
    if (done(mask, st)) return mask;
    if (!(mask & GPK_LL_B_OUTSIDE) && !row_covered<G>(B, A, lane)) mask |= GPK_LL_B_OUTSIDE;
    return mask;
}

// lanes per pair, pp::relation_group_size's rule: the lanes stride the coordinates of either column in turn, so the larger of the two
// mean coordinate counts decides
static inline int relation_group_size(const DevGeo& a, const DevGeo& b) {
    const int ga = lp::relation_group_size(a, a), gb = lp::relation_group_size(b, b);
    return ga > gb ? ga : gb;
}

}  // namespace ll
}  // namespace gpk
