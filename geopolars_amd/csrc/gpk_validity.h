// gpk_validity.h — is a polygonal row OGC-valid, is a lineal row simple: the device routines of gpk_validity / gpk_is_simple
// (include/geopolars_hip.h states the ten codes and the `where` of each).  The questions of gpk_polyrel.h, asked inside one geometry.
//
// A row is its live sequences: the non-empty rings of its non-empty members (a member without rings or with an empty shell is
// ignored, as the relation calls ignore it), or the non-empty members of a lineal row.  Its coordinates are one contiguous range, a
// segment is named by the index of its first coordinate, zero-length segments take part in nothing.
//
//   codes 1, 2      one pass over the coordinates / the rings: the lowest non-finite coordinate; the lowest ring with fewer than 4
//                   coordinates or different ends.  They end the row: everything below reads closed rings of finite coordinates.
//   codes 3, 4      segment x segment.  meet(e, f) of two segments is nothing, one point x, or a piece of positive length: four exact
//                   orientations and, for collinear segments, coordinate comparisons.
//                     same ring: e and f are neighbours when every coordinate between them (round the closing vertex too) is equal;
//                       neighbours may share the one point, anything else is code 3.  A ring of equal coordinates only: code 3.
//                     two rings R, S: a piece is code 4.  One point x that is inside both segments is a crossing: code 4.  Otherwise x
//                       is a coordinate of e or f; R leaves x in two directions (its neighbouring distinct vertices, or both ends of e
//                       when x is inside e) and S has a sector there (cont::dir_at_vertex at a vertex of S, the side of f inside f):
//                       code 4 unless both directions lie strictly on the same side — else the rings only touch at x.
//                   where = the lowest first segment of such a pair (every segment through a crossing point is in one).
//                   Lines: the same within a member (a closed member's first and last segments are neighbours); two members may share
//                   a point x only when x is an end point of both, and a closed member has none.
//   codes 5, 6, 7   no two rings cross now, so a ring lies on one side of another as a whole: cont::ring_rel (first vertex off the
//                   other ring, else first edge piece off it).  5: a hole outside its shell; 6: a hole inside another hole of its
//                   member; 7: the shell of one member inside the shell and outside every hole of another.
//   code 8          only when the segment pass saw two rings touch: per member, union-find over its rings.  Every distinct touch
//                   point is a coordinate of one of the rings through it; it is handled at the lowest ring that has it as a
//                   coordinate (once: copies of a ring's start at its end are left out), which is joined with every other ring
//                   through it.  Joining two rings that are joined already is a cycle of the ring / touch-point graph: the interior
//                   is cut.  The lanes look for the rings through a point together, lane 0 alone runs find / union on the scratch
//                   (`parent`, one int per ring of the column).  Cost, paid only by rows with a touch: every coordinate of every
//                   ring of a member against every segment of its other rings, (sum over ring pairs R, S of |R| |S|) / G trips — for
//                   a 10^4-coordinate shell touched by a 100-coordinate hole 2 x 10^6 / 16 on the 16 lanes a large row has.
//
// Schedules.  G lanes per row (G = 4 or 16 from the column's mean coordinate count, validity_group_size) for rows of at most
// VAL_BLOCK_COORDS coordinates: the outer segment is the same on all lanes, the inner one strided; every branch around a reduction
// is group-uniform.  Cost: n^2 / (2 G) box tests per lane for a row of n coordinates, orientations only where boxes meet.
// Rows above VAL_BLOCK_COORDS are queued by that kernel and taken by a work-group each: the row's box is cut into K equal strips
// along its longer axis, K = n / VAL_SEGS_PER_STRIP (at most VAL_STRIPS_MAX), every segment is entered in LDS under each strip its
// extent meets (count, scan, fill: 3 n LDS atomics), and only pairs that share a strip are tested, each in the first strip they
// share.  A ring crosses a strip a few times, so the lists hold T = n + c K entries (c: how often the boundary runs to and fro along
// the axis; 2 for a convex ring) and the tests number about T^2 / K = 8 (1 + c / 8)^2 n instead of n^2 / 2: 10^5 against 5 x 10^7 for
// a 10^4-coordinate shell.  When T exceeds VAL_ENTRIES the strips are doubled in width until it fits; a ROW whose segments — of all
// its rings together — do not fit even in one strip (more than VAL_ENTRIES of them) takes the all-pairs loop with the whole
// work-group: n^2 / 512 box tests per thread, 2 x 10^7 for a row of 10^5 coordinates.  Codes 5 - 8 of such a
// row run on the first 16 lanes: one ring_rel per hole is (coordinates of the shell) / 16 trips.
#pragma once

#include "gpk_contains.h"
#include "gpk_device.h"
#include "gpk_linearea.h"
#include "gpk_pairdist.h"
#include "gpk_polyrel.h"

namespace gpk {
namespace val {

constexpr int VAL_G_SMALL = 4, VAL_G_LARGE = 16;
constexpr double VAL_G_MEAN = 32.0;     // columns of at least this many coordinates a row on average take VAL_G_LARGE
constexpr int VAL_BLOCK_COORDS = 512;   // rows of more coordinates take the work-group path
constexpr int VAL_BLOCK_THREADS = 256;
constexpr int VAL_SEGS_PER_STRIP = 8;   // K = segments / VAL_SEGS_PER_STRIP strips ...
constexpr int VAL_STRIPS_MAX = 1024;    // ... at most
constexpr int VAL_ENTRIES = 12288;      // LDS entries of the strip lists (48 KB)
constexpr int NONE = 0x7fffffff;

static inline int validity_group_size(const DevGeo& a) {
    const double m = a.n_geoms > 0 ? (double)a.n_coords / (double)a.n_geoms : 0.0;
    return m >= VAL_G_MEAN ? VAL_G_LARGE : VAL_G_SMALL;
}

// ---- reductions: G lanes of a wave, or the whole work-group through LDS ----------------------------------------------------------
template <int G>
struct GroupCtx {
    static constexpr int T = G;
    int lane;
    __device__ __forceinline__ int imin(int v) const { return lp::group_imin<G>(v); }
    __device__ __forceinline__ int ior(int v) const { return dev::group_or<G>(v); }
};
struct BlockCtx {
    static constexpr int T = VAL_BLOCK_THREADS;
    int lane;
    int* slot;  // LDS
    __device__ __forceinline__ int imin(int v) const {
        if (lane == 0) *slot = NONE;
        __syncthreads();
        if (v != NONE) atomicMin(slot, v);
        __syncthreads();
        const int r = *slot;
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ int ior(int v) const {
        if (lane == 0) *slot = 0;
        __syncthreads();
        if (v) atomicOr(slot, v);
        __syncthreads();
        const int r = *slot;
        __syncthreads();
        return r;
    }
};

// ---- the row --------------------------------------------------------------------------------------------------------------------
struct Row {
    const double2* xy;
    const int32_t* so;       // sequence offsets
    const int32_t* part_off; // MULTIPOLYGON: ring offsets of the members [p0, p1]; else nullptr
    int p0, p1;
    int s0, s1, c0, c1;
    bool poly;
};
__device__ __forceinline__ Row polygon_row(const DevGeo& g, int64_t i) {
    const RowSeqs q = pp::ring_seqs(g, i);
    Row r{q.xy, q.so, nullptr, 0, 0, q.s0, q.s1, q.c0, q.c1, true};
    if (g.type == GPK_GEOM_MULTIPOLYGON) {
        r.part_off = g.part_off;
        r.p0 = g.geom_off[i];
        r.p1 = g.geom_off[i + 1];
    }
    return r;
}
__device__ __forceinline__ Row line_row(const DevGeo& g, int64_t i) {
    const RowSeqs q = lp::line_seqs(g, i);
    return Row{q.xy, q.so, nullptr, 0, 0, q.s0, q.s1, q.c0, q.c1, false};
}
// the rings [r0, r1) of the member that holds sequence s
__device__ inline void member_of(const Row& r, int s, int& r0, int& r1) {
    if (!r.part_off) {
        r0 = r.s0;
        r1 = r.s1;
        return;
    }
    const int p = seq_of(r.part_off, r.p0, r.p1, s);
    r0 = r.part_off[p];
    r1 = r.part_off[p + 1];
}
// a sequence that counts: it has coordinates and, in a polygonal row, its member's shell has
__device__ inline bool live(const Row& r, int s) {
    if (r.so[s + 1] <= r.so[s]) return false;
    if (!r.poly) return true;
    int r0, r1;
    member_of(r, s, r0, r1);
    return r.so[r0 + 1] > r.so[r0];
}
__device__ __forceinline__ bool finite2(double2 p) { return fabs(p.x) < INFINITY && fabs(p.y) < INFINITY; }  // (false for NaN)

// ---- codes 1 and 2, and the ring of equal coordinates (code 3) --------------------------------------------------------------------
struct Shape {
    int bad_coord, bad_ring, flat_ring;  // coordinate indices, NONE: none
};
template <class Ctx>
__device__ inline Shape row_shape(const Row& r, const Ctx& cx) {
    Shape sh{NONE, NONE, NONE};
    for (int c = r.c0 + cx.lane; c < r.c1; c += Ctx::T)
        if (!finite2(r.xy[c]) && live(r, seq_of(r.so, r.s0, r.s1, c))) {
            sh.bad_coord = c;  // (the lane's lowest: it walks upwards)
            break;
        }
    sh.bad_coord = cx.imin(sh.bad_coord);
    if (sh.bad_coord != NONE || !r.poly) return sh;
    for (int s = r.s0 + cx.lane; s < r.s1; s += Ctx::T) {
        if (!live(r, s)) continue;
        const int a = r.so[s], n = r.so[s + 1] - a;
        if (n < 4 || !cont::same_xy(r.xy[a], r.xy[a + n - 1])) {
            sh.bad_ring = sh.bad_ring < a ? sh.bad_ring : a;
            continue;
        }
        int k = 1;
        while (k < n && cont::same_xy(r.xy[a + k], r.xy[a])) ++k;
        if (k == n) sh.flat_ring = sh.flat_ring < a ? sh.flat_ring : a;
    }
    sh.bad_ring = cx.imin(sh.bad_ring);
    sh.flat_ring = cx.imin(sh.flat_ring);
    return sh;
}

// ---- segment x segment ------------------------------------------------------------------------------------------------------------
// what the closed segments ab and cd (a != b, c != d) share: 0 nothing, 2 a piece of positive length, 1 one point — then `proper`:
// it is inside both segments, else x = it (a coordinate of one of them)
__device__ inline int seg_meet(double2 a, double2 b, double2 c, double2 d, double2& x, bool& proper) {
    const int o1 = cont::orient(a, b, c), o2 = cont::orient(a, b, d);
    proper = false;
    if (o1 == 0 && o2 == 0) {
        const bool by_x = a.x != b.x;
        const double a1 = by_x ? a.x : a.y, b1 = by_x ? b.x : b.y, c1 = by_x ? c.x : c.y, d1 = by_x ? d.x : d.y;
        const double lo = fmax(fmin(a1, b1), fmin(c1, d1)), hi = fmin(fmax(a1, b1), fmax(c1, d1));
        if (lo < hi) return 2;
        if (lo > hi) return 0;
        x = a1 == lo ? a : b;
        return 1;
    }
    if (o1 * o2 > 0) return 0;
    const int o3 = cont::orient(c, d, a), o4 = cont::orient(c, d, b);
    if (o3 * o4 > 0) return 0;
    if (o1 == 0)
        x = c;
    else if (o2 == 0)
        x = d;
    else if (o3 == 0)
        x = a;
    else if (o4 == 0)
        x = b;
    else
        proper = true;
    return 1;
}

// segments i < j of one sequence [q0, q1) that meet: are they neighbours (nothing but equal coordinates between them)
__device__ inline bool neighbours(const double2* xy, int q0, int q1, int i, int j) {
    const double2 a = xy[i], b = xy[i + 1], c = xy[j], d = xy[j + 1];
    if (cont::same_xy(b, c)) {
        bool adj = true;
        for (int k = i + 2; k < j && adj; ++k) adj = cont::same_xy(xy[k], b);
        if (adj) return true;
    }
    if (!cont::same_xy(d, a)) return false;
    for (int k = j + 2; k < q1; ++k)
        if (!cont::same_xy(xy[k], a)) return false;
    for (int k = q0; k < i; ++k)
        if (!cont::same_xy(xy[k], a)) return false;
    return true;
}

// the two directions in which the closed ring [q0, q1) leaves x, a point of its segment i (a -> b)
__device__ inline void ring_dirs(const double2* xy, int q0, int q1, int i, double2 x, double2& w1, double2& w2) {
    const cont::Ring R{xy + q0, q1 - q0 - 1, 1};
    const double2 a = xy[i], b = xy[i + 1];
    w1 = a;
    w2 = b;
    if (cont::same_xy(x, a))
        w1 = R.v[cont::prev_distinct(R, i - q0)];
    else if (cont::same_xy(x, b))
        w2 = R.v[cont::next_distinct(R, (i + 1 - q0) % R.m)];
}
// the side of the closed ring [q0, q1) at x, a point of its segment j (c -> d), on which the direction x -> w lies
__device__ inline int ring_side_at(const double2* xy, int q0, int q1, int j, double2 x, double2 w) {
    const cont::Ring S{xy + q0, q1 - q0 - 1, 1};
    const double2 c = xy[j], d = xy[j + 1];
    if (cont::same_xy(x, c)) return cont::dir_at_vertex(S, j - q0, w);
    if (cont::same_xy(x, d)) return cont::dir_at_vertex(S, (j + 1 - q0) % S.m, w);
    const int o = cont::orient(c, d, w);
    return o > 0 ? cont::DIR_IN : (o < 0 ? cont::DIR_OUT : 0);
}

struct Found {
    int self, cross, touch;  // lowest segment of a code-3 pair, of a code-4 pair (lines: of two members' pair); rings touched
};

// One pair of segments i < j of the row; i lies in the live sequence si = [i0, i1).  Box test first, the sequences after it.
__device__ inline void pair_test(const Row& r, int si, int i0, int i1, int i, double2 a, double2 b, int j, Found& f) {
    const double2 c = r.xy[j], d = r.xy[j + 1];
    if (fmax(c.x, d.x) < fmin(a.x, b.x) || fmin(c.x, d.x) > fmax(a.x, b.x) || fmax(c.y, d.y) < fmin(a.y, b.y) || fmin(c.y, d.y) > fmax(a.y, b.y))
        return;
    if (cont::same_xy(c, d)) return;
    const int sj = j < i1 ? si : seq_of(r.so, r.s0, r.s1, j);
    const int j0 = r.so[sj], j1 = r.so[sj + 1];
    if (j + 1 >= j1 || (sj != si && !live(r, sj))) return;  // (j: the last coordinate of its sequence)
    double2 x;
    bool proper;
    const int m = seg_meet(a, b, c, d, x, proper);
    if (m == 0) return;
    if (sj == si) {
        if (m == 2 || !neighbours(r.xy, i0, i1, i, j)) f.self = f.self < i ? f.self : i;
        return;
    }
    bool bad = m == 2 || proper;
    if (!bad && r.poly) {
        double2 w1, w2;
        ring_dirs(r.xy, i0, i1, i, x, w1, w2);
        const int s1 = ring_side_at(r.xy, j0, j1, j, x, w1), s2 = ring_side_at(r.xy, j0, j1, j, x, w2);
        bad = s1 == 0 || s2 == 0 || s1 != s2;
        if (!bad) f.touch = 1;
    } else if (!bad) {  // two members of a line: x must be an end point of both
        const bool end_i = !cont::same_xy(r.xy[i0], r.xy[i1 - 1]) && (cont::same_xy(x, r.xy[i0]) || cont::same_xy(x, r.xy[i1 - 1]));
        const bool end_j = !cont::same_xy(r.xy[j0], r.xy[j1 - 1]) && (cont::same_xy(x, r.xy[j0]) || cont::same_xy(x, r.xy[j1 - 1]));
        bad = !(end_i && end_j);
    }
    if (bad) f.cross = f.cross < i ? f.cross : i;
}

// every pair of the row, the inner segment strided over the lanes (the reductions are the caller's)
template <class Ctx>
__device__ inline void all_pairs(const Row& r, const Ctx& cx, Found& f) {
    for (int s = r.s0; s < r.s1; ++s) {
        if (!live(r, s)) continue;
        const int i0 = r.so[s], i1 = r.so[s + 1];
        for (int i = i0; i + 1 < i1; ++i) {
            const double2 a = r.xy[i], b = r.xy[i + 1];
            if (cont::same_xy(a, b)) continue;
            for (int j = i + 1 + cx.lane; j + 1 < r.c1; j += Ctx::T) pair_test(r, s, i0, i1, i, a, b, j, f);
        }
    }
}

// ---- codes 5 - 8 --------------------------------------------------------------------------------------------------------------------
__device__ inline int uf_find(int32_t* parent, int v) {
    while (parent[v] != v) {
        const int p = parent[parent[v]];
        parent[v] = p;
        v = p;
    }
    return v;
}

// does the member with rings [r0, r1) have a cycle in its ring / touch-point graph.  The lanes search the rings through a point
// together; the union-find itself runs on lane 0 alone, its verdict goes round the group.
template <int G>
__device__ inline bool member_cut(const Row& r, int r0, int r1, int32_t* parent, int lane) {
    if (lane == 0)
        for (int s = r0; s < r1; ++s) parent[s] = s;
    for (int s = r0; s < r1; ++s) {
        const int q0 = r.so[s];
        int q1 = r.so[s + 1] - 1;  // without the closing coordinate ...
        while (q1 > q0 + 1 && cont::same_xy(r.xy[q1 - 1], r.xy[q0])) --q1;  // ... and without copies of the start in front of it
        for (int vi = q0; vi < q1; ++vi) {
            const double2 v = r.xy[vi];
            if (vi > q0 && cont::same_xy(v, r.xy[vi - 1])) continue;  // (a simple ring visits a point once, but for repeats in a row)
            // a lower ring with a coordinate at v has handled the point
            int seen = 0;
            for (int t = r0; t < s && !seen; ++t) {
                const int t0 = r.so[t], m = r.so[t + 1] - t0 - 1;
                int hit = 0;
                for (int e = lane; e < m; e += G) hit |= cont::same_xy(r.xy[t0 + e], v) ? 1 : 0;
                seen = dev::group_or<G>(hit);
            }
            if (seen) continue;
            for (int t = r0; t < r1; ++t) {
                if (t == s) continue;
                const int t0 = r.so[t], m = r.so[t + 1] - t0 - 1;
                int on = 0;
                for (int e = lane; e < m; e += G) {
                    const double2 a = r.xy[t0 + e], b = r.xy[t0 + e + 1];
                    if (cont::same_xy(a, v))
                        on = 1;
                    else if (!cont::same_xy(a, b) && cont::strictly_between(v, a, b) && cont::orient(a, b, v) == 0)
                        on = 1;
                }
                if (!dev::group_or<G>(on)) continue;
                int cycle = 0;
                if (lane == 0) {
                    const int ra = uf_find(parent, s), rb = uf_find(parent, t);
                    cycle = ra == rb;
                    parent[rb] = ra;
                }
                if (dev::group_or<G>(cycle)) return true;
            }
        }
    }
    return false;
}

// the lowest of the codes 5 - 8 of a row that has none of 1 - 4, and its `where`; code 0: valid
template <int G>
__device__ inline int row_nesting(const DevGeo& g, const Row& r, int64_t row, bool touched, int32_t* parent, int lane, int& where) {
    int p0, p1;
    dev::geom_parts(g, row, p0, p1);
    where = NONE;
    // 5: a hole outside its shell
    for (int p = p0; p < p1; ++p) {
        int r0, r1;
        if (!lp::part_of(g, p, r0, r1) || r1 - r0 < 2) continue;
        cont::Ring sh;
        (void)cont::ring_init<G>(sh, g.xy + g.ring_off[r0], g.ring_off[r0 + 1] - g.ring_off[r0], lane);
        for (int h = r0 + 1; h < r1; ++h) {
            const int h0 = g.ring_off[h], hn = g.ring_off[h + 1] - h0;
            if (hn == 0) continue;
            if (cont::ring_rel<G>(g.xy + h0, hn - 1, sh, lane) == cont::REL_OUT) where = where < h0 ? where : h0;
        }
    }
    if (where != NONE) return GPK_INVALID_HOLE_OUTSIDE_SHELL;
    // 6: a hole inside another hole of its member
    for (int p = p0; p < p1; ++p) {
        int r0, r1;
        if (!lp::part_of(g, p, r0, r1) || r1 - r0 < 3) continue;
        for (int k = r0 + 1; k < r1; ++k) {
            const int k0 = g.ring_off[k], kn = g.ring_off[k + 1] - k0;
            if (kn == 0) continue;
            cont::Ring outer;
            (void)cont::ring_init<G>(outer, g.xy + k0, kn, lane);
            for (int h = r0 + 1; h < r1; ++h) {
                const int h0 = g.ring_off[h], hn = g.ring_off[h + 1] - h0;
                if (h == k || hn == 0) continue;
                if (cont::ring_rel<G>(g.xy + h0, hn - 1, outer, lane) == cont::REL_IN) where = where < h0 ? where : h0;
            }
        }
    }
    if (where != NONE) return GPK_INVALID_NESTED_HOLES;
    // 7: the shell of a member inside the shell and outside every hole of another one
    for (int pb = p0; pb < p1 && where == NONE; ++pb) {
        int b0, b1;
        if (!lp::part_of(g, pb, b0, b1)) continue;
        for (int pa = p0; pa < pb && where == NONE; ++pa) {
            int a0, a1;
            if (!lp::part_of(g, pa, a0, a1)) continue;
            for (int turn = 0; turn < 2 && where == NONE; ++turn) {  // B in A, then A in B
                const int i0 = turn ? a0 : b0, o0 = turn ? b0 : a0, o1 = turn ? b1 : a1;
                const double2* in_xy = g.xy + g.ring_off[i0];
                const int in_m = g.ring_off[i0 + 1] - g.ring_off[i0] - 1;
                bool inside = true;
                for (int k = o0; k < o1 && inside; ++k) {
                    const int k0 = g.ring_off[k], kn = g.ring_off[k + 1] - k0;
                    if (kn == 0) continue;
                    cont::Ring ring;
                    (void)cont::ring_init<G>(ring, g.xy + k0, kn, lane);
                    const int rel = cont::ring_rel<G>(in_xy, in_m, ring, lane);
                    inside = k == o0 ? rel == cont::REL_IN : rel != cont::REL_IN;
                }
                if (inside) where = g.ring_off[b0];
            }
        }
    }
    if (where != NONE) return GPK_INVALID_NESTED_MEMBERS;
    // 8: a member cut by rings that touch
    if (touched && parent) {
        for (int p = p0; p < p1; ++p) {
            int r0, r1;
            if (!lp::part_of(g, p, r0, r1) || r1 - r0 < 2) continue;
            if (member_cut<G>(r, r0, r1, parent, lane)) {
                where = g.ring_off[r0];
                return GPK_INVALID_DISCONNECTED_INTERIOR;
            }
        }
    }
    where = -1;
    return GPK_VALID;
}

// the code of a row from the three stages; `where` follows the header
__device__ __forceinline__ int early_code(const Shape& sh, int& where) {
    if (sh.bad_coord != NONE) {
        where = sh.bad_coord;
        return GPK_INVALID_COORDINATE;
    }
    if (sh.bad_ring != NONE) {
        where = sh.bad_ring;
        return GPK_INVALID_RING_SHAPE;
    }
    return GPK_VALID;
}
__device__ __forceinline__ int pair_code(const Shape& sh, const Found& f, int& where) {
    const int self = f.self < sh.flat_ring ? f.self : sh.flat_ring;
    if (self != NONE) {
        where = self;
        return GPK_INVALID_RING_SELF_INTERSECTION;
    }
    if (f.cross != NONE) {
        where = f.cross;
        return GPK_INVALID_RINGS_CROSS;
    }
    return GPK_VALID;
}

}  // namespace val
}  // namespace gpk
