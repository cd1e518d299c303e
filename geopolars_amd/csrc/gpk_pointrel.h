// gpk_pointrel.h — how a punctual geometry lies to a geometry of any family: the 4-bit mask of gpk_point_relation
// (include/geopolars_hip.h).  A = a POINT / MULTIPOINT row, the finite set of its points.  B = a row of any of
// the six families.
//   GPK_PT_INTERIOR  1   a point of A lies in the interior of B
//   GPK_PT_BOUNDARY  2   a point of A lies on the boundary of B
//   GPK_PT_EXTERIOR  4   a point of A is no point of B
//   GPK_PT_B_OUTSIDE 8   B has a point that is no point of A
// This is DE-9IM with dim(A) = 0 and an empty boundary of A: II, IB, IE are the bits 1, 2, 4, and bit 8 is "EI or EB non-empty" (EE
// is always non-empty, the row of A's boundary is empty).  Every named predicate is a function of the mask and of dim(B) (predicate_of).
// For two punctual rows mask(B, A) is mask(A, B) with the bits 4 and 8 swapped.
//
// Interior and boundary of B are those of the sibling relations, by reference:
//   punctual B    every point is interior, there is no boundary.  Bit 8: some point of B equals no point of A, by exact coordinate
//                 comparison; duplicates and member order do not matter.
//   lineal B      the closed point set of its segments and coordinates with the mod-2 boundary of gpk_lineline.h: every non-empty
//                 member counts its first and last coordinate once each, a point counted an odd number of times is a boundary point.
//                 A point is on B when it equals a coordinate or lies in a segment's box with orient == 0; its status is the parity of
//                 the member ends equal to it, counted on the fly (as ll::ends_at).  Bit 8 unless every member is degenerate (one
//                 coordinate, or equal coordinates) and each of those points is a point of A.  Nothing assumes B is simple.
//   polygonal B   the point sets of gpk_polyrel.h: boundary = on a ring; interior = inside a part's shell, outside its holes and on no
//                 ring; exterior = outside every part or strictly inside a hole.  For an OGC-valid row (holes inside their shell and
//                 not nested, interiors of parts disjoint, rings touching at points at most) a point on no ring is interior exactly
//                 when a ray from it crosses the rings of the row an odd number of times, so ONE pass over all edges of the row
//                 decides: no ring is told from another.  Bit 8 is always set.  A non-empty ring that fails the ring rule of `contains`
//                 (cont::ring_init: fewer than 4 coordinates, unclosed, no turning lexicographically smallest vertex) makes the row
//                 unusable.  For an invalid polygon the mask is unspecified and the routine terminates.
// Rows, on either side: null, no coordinate, a NaN or infinite coordinate (a POINT with NaN is the empty point): mask 0.  Empty
// members are ignored.  A usable pair never has mask 0.  The masks that can occur:
//   punctual B     1, 5, 9, 12, 13
//   polygonal B    9 .. 15
//   lineal B       9 .. 15, and for rows all of whose members are degenerate additionally 1, 5
// (tests/pointrel_ref.py confirms the list by brute force).
//
// Schedule.  G lanes work on one pair: the point of A under test is the same on all of them, B's coordinates and segments are strided
// over the lanes, every reduction sits in group-uniform control flow.  A point outside B's box is exterior at once.  Cost per pair with
// m points against n coordinates whose boxes meet: m n / G element tests (a coordinate comparison, a box test, one orientation where
// the point is in a segment's box or, for a polygon, level with an edge), one pass over the member ends per point that lies on a
// line, and n m / G comparisons more for bit 8 of a finite B when nothing stopped the pair earlier.  Pairs with m n > PT_LARGE_COST
// are finished by a 256-lane work-group that stages B through LDS (gpk_pointrel.hip).
//
// The routine is plain C++ over a lane-group size and an orientation functor (as gpk_lineclip.h and gpk_overlay.h): the kernels
// instantiate it with dev::orient2d at G = 4 / 16, tests/pointrel_host_driver.cpp with an exact integer orientation at G = 1.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/geopolars_hip.h"
#include "gpk_frac.h"

#if defined(__HIPCC__)
#include "gpk_device.h"
#define GPK_PT_FN __device__ inline
#define GPK_PT_HD __host__ __device__ inline
#else
#define GPK_PT_FN inline
#define GPK_PT_HD inline
#endif

namespace gpk {
namespace pt {

constexpr int INTERIOR = GPK_PT_INTERIOR, BOUNDARY = GPK_PT_BOUNDARY, EXTERIOR = GPK_PT_EXTERIOR, B_OUTSIDE = GPK_PT_B_OUTSIDE;
constexpr int PT_ALL = 15;
constexpr int PENDING = 16;  // (between the two launches of a listed pair: B is a finite set and bit 8 is still open)
enum {
    PRED_INTERSECTS = GPK_PT_PRED_INTERSECTS,
    PRED_WITHIN = GPK_PT_PRED_WITHIN,
    PRED_CONTAINS = GPK_PT_PRED_CONTAINS,
    PRED_COVERED_BY = GPK_PT_PRED_COVERED_BY,
    PRED_COVERS = GPK_PT_PRED_COVERS,
    PRED_CROSSES = GPK_PT_PRED_CROSSES,
    PRED_TOUCHES = GPK_PT_PRED_TOUCHES,
    PRED_OVERLAPS = GPK_PT_PRED_OVERLAPS,
    PRED_EQUALS = GPK_PT_PRED_EQUALS
};

// pairs with n_A * n_B above this are listed for the work-group schedule
constexpr int64_t PT_LARGE_COST = PD_LARGE_COST;  // a first value, not swept

struct alignas(16) P2 {
    double x, y;
};

// When a caller needs less than the mask: stop as soon as one of `any` is set or all of `all` are.  {0, PT_ALL}: the full mask.
struct Stop {
    int any, all;
};
GPK_PT_HD bool done(int mask, Stop st) { return (mask & st.any) != 0 || (mask & st.all) == st.all; }

// the predicate ids of gpk_point_relation_join over the mask and the dimension of B's family (0, 1, 2)
GPK_PT_HD bool predicate_of(int mask, int pred, int dim_b) {
    switch (pred) {
    case PRED_INTERSECTS: return (mask & 3) != 0;
    case PRED_WITHIN: return (mask & 1) && !(mask & 4);
    case PRED_CONTAINS: return (mask & 1) && !(mask & 8);
    case PRED_COVERED_BY: return (mask & 3) && !(mask & 4);
    case PRED_COVERS: return (mask & 3) && !(mask & 8);
    case PRED_CROSSES: return dim_b >= 1 && (mask & 1) && (mask & 4);
    case PRED_TOUCHES: return (mask & 2) && !(mask & 1);
    case PRED_OVERLAPS: return dim_b == 0 && (mask & 13) == 13;
    case PRED_EQUALS: return (mask & 1) && !(mask & 12);
    default: return false;
    }
}
// can the predicate hold for a B of this dimension at all
inline bool can_hold(int pred, int dim_b) { return pred == PRED_CROSSES ? dim_b >= 1 : (pred == PRED_OVERLAPS ? dim_b == 0 : true); }
// the bits that settle a predicate before the mask is complete
inline Stop stop_of(int pred) {
    switch (pred) {
    case PRED_INTERSECTS: return Stop{3, PT_ALL};
    case PRED_WITHIN:
    case PRED_COVERED_BY: return Stop{4, PT_ALL};
    case PRED_CONTAINS:
    case PRED_COVERS: return Stop{8, PT_ALL};
    case PRED_CROSSES: return Stop{0, 5};
    case PRED_TOUCHES: return Stop{1, PT_ALL};
    case PRED_OVERLAPS: return Stop{0, 13};
    case PRED_EQUALS: return Stop{12, PT_ALL};
    default: return Stop{0, PT_ALL};
    }
}
// "B pred A" as a predicate of (A, B): within <-> contains, covered_by <-> covers, the rest read the same both ways
inline int transposed(int pred) {
    switch (pred) {
    case PRED_WITHIN: return PRED_CONTAINS;
    case PRED_CONTAINS: return PRED_WITHIN;
    case PRED_COVERED_BY: return PRED_COVERS;
    case PRED_COVERS: return PRED_COVERED_BY;
    default: return pred;
    }
}

// One row: coordinates [c0, c1) of xy; sequences [s0, s1) of `so` (members of a line, rings of a polygon; nullptr for a punctual row);
// dim: the dimension of the row's FAMILY
struct Row {
    const P2* xy;
    const int32_t* so;
    int s0, s1, c0, c1, dim;
};

GPK_PT_FN bool same(P2 a, P2 b) { return a.x == b.x && a.y == b.y; }
GPK_PT_FN bool finite2(P2 p) { return p.x - p.x == 0.0 && p.y - p.y == 0.0; }

// reductions over the G lanes of a pair (G = 1: one lane, anywhere)
template <int G>
GPK_PT_FN int lanes_or(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return dev::group_or<G>(v);
#else
    return v;
#endif
}
template <int G>
GPK_PT_FN int lanes_sum(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return dev::group_sum<G>(v);
#else
    return v;
#endif
}
template <int G>
GPK_PT_FN int lanes_imin(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return dev::group_allreduce<G>(v, [](int a, int b) { return a < b ? a : b; });
#else
    return v;
#endif
}
template <int G>
GPK_PT_FN double lanes_min(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return dev::group_min<G>(v);
#else
    return v;
#endif
}
template <int G>
GPK_PT_FN double lanes_max(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return dev::group_max<G>(v);
#else
    return v;
#endif
}

// What one point has seen of B so far: on a coordinate or a segment, the parity of the crossings of its ray (polygonal B), the
// member ends equal to it (counted where the caller knows them: the work-group schedule).
struct Acc {
    int on, cross, ends;
};
// One element of B against the point p: the coordinate c and the segment c -> d that starts there (d == c: none); `ends_here`: how
// many member ends c is.  orient(u, v, w): the exact sign of cross(v - u, w - u).
template <class Orient>
GPK_PT_FN void see(Acc& a, P2 p, P2 c, P2 d, int ends_here, int dim, Orient orient) {
    if (same(c, p)) {
        a.on = 1;
        a.ends += ends_here;
        return;
    }
    if (dim == 0 || same(c, d)) return;
    const bool in_box = p.x >= fmin(c.x, d.x) && p.x <= fmax(c.x, d.x) && p.y >= fmin(c.y, d.y) && p.y <= fmax(c.y, d.y);
    if (dim == 1) {
        if (in_box && orient(c, d, p) == 0) a.on = 1;
        return;
    }
    // the ray from p towards +x against the edge, half-open in y: an edge level with p counts once at its lower end
    const bool up = c.y <= p.y && p.y < d.y, down = d.y <= p.y && p.y < c.y;
    if (!in_box && !up && !down) return;
    const int o = orient(c, d, p);
    if (o == 0) {
        if (in_box) a.on = 1;
    } else if ((up && o > 0) || (down && o < 0)) {
        a.cross ^= 1;
    }
}
// the bit of a point from what it saw of the whole of B
GPK_PT_FN int bit_of(int on, int cross, int ends, int dim) {
    if (dim == 0) return on ? INTERIOR : EXTERIOR;
    if (dim == 1) return on ? ((ends & 1) ? BOUNDARY : INTERIOR) : EXTERIOR;
    return on ? BOUNDARY : ((cross & 1) ? INTERIOR : EXTERIOR);
}

// the ring rule of `contains` (cont::ring_init) for a ring of finite coordinates: at least 4 of them, closed, and a turn at the
// lexicographically smallest vertex
template <int G, class Orient>
GPK_PT_FN bool ring_usable(const P2* v, int n, int lane, Orient orient) {
    if (n < 4 || !same(v[0], v[n - 1])) return false;
    const int m = n - 1;
    double bx = INFINITY, by = INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < m; i += G) {
        const P2 p = v[i];
        if (p.x < bx || (p.x == bx && p.y < by)) {
            bx = p.x;
            by = p.y;
            bi = i;
        }
    }
    const double gx = lanes_min<G>(bx);
    const double gy = lanes_min<G>(bx == gx ? by : INFINITY);
    const int k = lanes_imin<G>((bx == gx && by == gy) ? bi : 0x7fffffff);
    if (k == 0x7fffffff) return false;
    int ip = -1, iq = -1;
    for (int t = 1; t < m && ip < 0; ++t)
        if (!same(v[(k - t + m) % m], v[k])) ip = (k - t + m) % m;
    for (int t = 1; t < m && iq < 0; ++t)
        if (!same(v[(k + t) % m], v[k])) iq = (k + t) % m;
    if (ip < 0 || iq < 0) return false;
    return orient(v[ip], v[k], v[iq]) != 0;
}

// the row's coordinates are finite (else false), and their box
template <int G>
GPK_PT_FN bool row_box(const Row& r, int lane, P2& lo, P2& hi) {
    double lx = INFINITY, ly = INFINITY, hx = -INFINITY, hy = -INFINITY;
    int bad = 0;
    for (int c = r.c0 + lane; c < r.c1; c += G) {
        const P2 v = r.xy[c];
        bad |= finite2(v) ? 0 : 1;
        lx = fmin(lx, v.x);
        ly = fmin(ly, v.y);
        hx = fmax(hx, v.x);
        hy = fmax(hy, v.y);
    }
    if (lanes_or<G>(bad)) return false;
    lo = P2{lanes_min<G>(lx), lanes_min<G>(ly)};
    hi = P2{lanes_max<G>(hx), lanes_max<G>(hy)};
    return true;
}

// What is known of a pair before a point of A is judged: whether either row is unusable (mask 0, settled), bit 8 of a B that is no
// finite set, boxes that are apart (12, settled).  b_finite: B is a finite set of points, its bit 8 needs the set comparison.
struct Pre {
    int mask;
    bool settled, b_finite;
    P2 lo_b, hi_b;
};
template <int G, class Orient>
GPK_PT_FN Pre prepare(const Row& A, const Row& B, int lane, Stop st, Orient orient) {
    Pre pre{0, true, false, P2{0.0, 0.0}, P2{0.0, 0.0}};
    if (A.c1 <= A.c0 || B.c1 <= B.c0) return pre;
    P2 lo_a, hi_a;
    if (!row_box<G>(A, lane, lo_a, hi_a) || !row_box<G>(B, lane, pre.lo_b, pre.hi_b)) return pre;
    if (B.dim == 2) {
        for (int s = B.s0; s < B.s1; ++s) {
            const int c0 = B.so[s], n = B.so[s + 1] - c0;
            if (n > 0 && !ring_usable<G>(B.xy + c0, n, lane, orient)) return pre;
        }
        pre.mask = B_OUTSIDE;
    } else if (B.dim == 1) {
        int nd = 0;
        for (int s = B.s0; s < B.s1; ++s)
            for (int j = B.so[s] + lane; j + 1 < B.so[s + 1]; j += G) nd |= same(B.xy[j], B.xy[j + 1]) ? 0 : 1;
        if (lanes_or<G>(nd))
            pre.mask = B_OUTSIDE;
        else
            pre.b_finite = true;
    } else {
        pre.b_finite = true;
    }
    if (hi_a.x < pre.lo_b.x || lo_a.x > pre.hi_b.x || hi_a.y < pre.lo_b.y || lo_a.y > pre.hi_b.y) {
        pre.mask = EXTERIOR | B_OUTSIDE;
        return pre;
    }
    pre.settled = done(pre.mask, st);
    return pre;
}

// the bit of the point p (the same on every lane) against the usable row B
template <int G, class Orient>
GPK_PT_FN int point_bit(P2 p, const Row& B, int lane, Orient orient) {
    Acc acc{0, 0, 0};
    if (B.dim == 0) {
        for (int j = B.c0 + lane; j < B.c1; j += G) acc.on |= same(B.xy[j], p) ? 1 : 0;
        return lanes_or<G>(acc.on) ? INTERIOR : EXTERIOR;
    }
    for (int s = B.s0; s < B.s1; ++s) {
        const int c1 = B.so[s + 1];
        for (int j = B.so[s] + lane; j < c1; j += G) {
            const P2 c = B.xy[j];
            see(acc, p, c, j + 1 < c1 ? B.xy[j + 1] : c, 0, B.dim, orient);
        }
    }
    const int on = lanes_or<G>(acc.on);
    if (B.dim == 2) return bit_of(on, lanes_sum<G>(acc.cross), 0, 2);
    if (!on) return EXTERIOR;
    int ends = 0;  // the member ends equal to p, counted now that p is known to lie on B
    for (int s = B.s0 + lane; s < B.s1; s += G) {
        const int c0 = B.so[s], c1 = B.so[s + 1];
        if (c1 > c0) ends += (same(B.xy[c0], p) ? 1 : 0) + (same(B.xy[c1 - 1], p) ? 1 : 0);
    }
    return bit_of(1, 0, lanes_sum<G>(ends), 1);
}

// The rest of a pair that `prepare` did not settle.  ONE: A is a single point (a POINT column): no outer loop, no set comparison.
template <int G, bool ONE, class Orient>
GPK_PT_FN int finish(const Row& A, const Row& B, const Pre& pre, int lane, Stop st, Orient orient) {
    int mask = pre.mask;
    const P2 lo = pre.lo_b, hi = pre.hi_b;
    if (ONE) {
        const P2 p = A.xy[A.c0];
        mask |= (p.x < lo.x || p.x > hi.x || p.y < lo.y || p.y > hi.y) ? EXTERIOR : point_bit<G>(p, B, lane, orient);
        if (pre.b_finite && !done(mask, st)) {
            int other = 0;
            for (int j = B.c0 + lane; j < B.c1; j += G) other |= same(B.xy[j], p) ? 0 : 1;
            if (lanes_or<G>(other)) mask |= B_OUTSIDE;
        }
        return mask;
    }
    for (int c = A.c0; c < A.c1; ++c) {
        const P2 p = A.xy[c];
        if (c > A.c0 && same(p, A.xy[c - 1])) continue;  // (decided with the point before it)
        mask |= (p.x < lo.x || p.x > hi.x || p.y < lo.y || p.y > hi.y) ? EXTERIOR : point_bit<G>(p, B, lane, orient);
        if (done(mask, st)) return mask;
    }
    if (pre.b_finite) {  // B is a finite set: is each of its points a point of A
        for (int j = B.c0; j < B.c1; ++j) {
            const P2 q = B.xy[j];
            if (j > B.c0 && same(q, B.xy[j - 1])) continue;
            int found = 0;
            for (int c = A.c0 + lane; c < A.c1; c += G) found |= same(A.xy[c], q) ? 1 : 0;
            if (!lanes_or<G>(found)) {
                mask |= B_OUTSIDE;
                break;
            }
        }
    }
    return mask;
}

// The mask of the punctual row A against the row B.  With `st` the work ends as soon as the bits a caller needs are settled (the mask
// is then partial).  Same value on every lane of the group.
template <int G, bool ONE, class Orient>
GPK_PT_FN int point_mask_group(const Row& A, const Row& B, int lane, Stop st, Orient orient) {
    const Pre pre = prepare<G>(A, B, lane, st, orient);
    return pre.settled ? pre.mask : finish<G, ONE>(A, B, pre, lane, st, orient);
}

}  // namespace pt
}  // namespace gpk
