// gpk_triangulate.h — the rule of gpk_triangulate: exact ear clipping of a polygonal row, holes and touching rings included
// (include/geopolars_hip.h states the contract; DESIGN.md section 4.3p the schedule).
//
// Every decision is the exact sign of an orientation (tri::orient: Shewchuk's stage-A filter, then expansion arithmetic on the input
// coordinates) or a coordinate comparison, and every choice among candidates goes to the lowest node number: the answer is a function
// of the figure, not of the placement, the lane count or the schedule.
//
// Nodes.  A row of n coordinates in r rings owns cap = n + 3 r node slots — and as many triangle slots: its SHARE.  A node is a
// position (cached), the coordinate index it stands for, its two neighbours and a tag (the ring number while rings are merged, the
// ear state while ears are clipped).  Per row:
//   1 build    every non-empty ring of every non-empty member: closing coordinate and consecutive repeats dropped (the first of a
//              run stays, the ring's first coordinate stands for the closing one), the ring rule checked (at least 4 coordinates,
//              closed, finite, 3 distinct positions left, a non-zero turn at the lowest (x, y) node), the shell turned
//              counter-clockwise and the holes clockwise by swapping neighbours: the interior is on the left of every edge.
//   2 split    for every original node w and every edge of ANOTHER ring of the row — of any member — that holds w in its open
//              interior, a node with w's coordinate index goes into that edge.  Edges are the current ones, so several touches of
//              one edge come out in order along it with no sorting.  Without it a hole that touches a shell edge mid-segment could
//              not be finished, and two members that touch would leave a T-junction.
//   per member:
//   3 merge    holes in the order of their lowest (x, y) node M.  A loop node at M's position whose left cone strictly holds both
//              neighbours of M: spliced there, no new node (a bridge of length zero).  Otherwise the lowest loop node V with M
//              strictly in V's left cone, V strictly in M's, and the closed segment MV free of every edge of the member except the
//              edges that end at M's or V's position — such an edge rejects V only when its far end lies on the open bridge.
//              Splice V M .. hole .. M' V': two new nodes a hole.
//   4 clip     the lowest node that is, or may be, an ear is taken.  b with neighbours a, c is an ear when orient(a, b, c) > 0; c
//              lies strictly in a's left cone or on the open ray from a through a's other neighbour, likewise a at c; and no other
//              live node lies in the closed triangle — a node AT a corner blocks only when one of its neighbours lies strictly
//              inside the triangle's angle there.  Ear states are cached: a clip re-opens only its two neighbours.  A cached "not
//              an ear" can be stale (a clip elsewhere may have freed the triangle); it is only ever conservative, and when no
//              candidate is left all of them are re-opened once before the row is given up.
//   5 spikes   a diagonal that runs along an existing edge through a pinch point leaves a, b, c with a and c at one position: b
//              and c are removed without a triangle, at the junction of every clip, until none is left there.
// Bounds: every loop runs at most cap (or a small multiple of cap) times; a row whose nodes or triangles would pass cap, whose
// holes find no bridge or whose loop runs out of ears is GPK_TRI_FAILED with zero triangles.  For a valid row the node count is at
// most n' + s + 2 h <= cap - 2 as long as the rings of ONE member touch each other only (their touch graph is a forest: at most
// 2 r - 2 incidences); members that touch each other at more than 3 r points can pass the share and fail.
//
// Schedule.  Everything is written once, for a context of T lanes: control flow is the same on every lane, lane 0 alone changes the
// list, the scans over nodes (touches, bridges, the triangle's content, the next candidate) are strided over the lanes and reduced.
// T = 1 is the host (tests/triangulate_host_driver.cpp), T = 4 / 16 a lane group with the list in its LDS slice, T = 256 a work-group
// with the list in LDS or, for a row of more than TRI_LDS_NODES slots, in global scratch (correct and slow).
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/geopolars_hip.h"  // GPK_TRI_*

#if defined(__HIPCC__)
#define GPK_TRI_FN __host__ __device__ inline
#define GPK_TRI_COLD __host__ __device__ __attribute__((noinline))
#else
#define GPK_TRI_FN inline
#define GPK_TRI_COLD __attribute__((noinline))
#endif

namespace gpk {
namespace tri {

constexpr int TRI_G_SMALL = 4, TRI_G_LARGE = 16;  // lanes a row in the lane-group kernel
constexpr double TRI_G_MEAN = 32.0;      // columns whose rows own at least this many node slots on average take TRI_G_LARGE
constexpr int TRI_SLICE_SMALL = 32;      // node slots of a group's LDS slice, TRI_G_SMALL (64 groups x 1 KB)
constexpr int TRI_SLICE_LARGE = 128;     // ... TRI_G_LARGE (16 groups x 4 KB)
constexpr int TRI_BLOCK_THREADS = 256;   // the work-group kernel takes the rows above the slice ...
constexpr int TRI_LDS_NODES = 5000;      // ... up to this many node slots (160 000 bytes of LDS); larger rows: the same routine, list in global scratch
constexpr int NODE_BYTES = 32;
constexpr int NONE = 0x7fffffff;
constexpr int T_LIVE = -1, T_EAR = -2, T_DEAD = -3, T_NOT = -4;  // tags of the clipping phase (ring numbers are >= 0)

struct P2 {
    double x, y;
};
struct Nodes {
    P2* xy;
    int *prv, *nxt, *cix, *tag;
};
// a row of a polygonal column: rings [s0, s1) over ring_off; part_off != nullptr: members [p0, p1) with rings part_off[p] ..
struct RowView {
    const P2* xy;
    const int32_t* ring_off;
    const int32_t* part_off;
    int p0, p1, s0, s1;
};
struct SeqCtx {  // one lane: the host
    static constexpr int T = 1;
    int lane;
    int imin(int v) const { return v; }
    int ior(int v) const { return v; }
    double dmin(double v) const { return v; }
    void sync() const {}
};

// ---- exact orientation (the arithmetic of dev::orient2d, host-compilable) ----------------------------------------------------------
GPK_TRI_COLD int orient_exact(double ax, double ay, double bx, double by, double cx, double cy) {
    const double f[12] = {ax, by, -ax, cy, -cx, by, -ay, bx, ay, cx, cy, bx};
    double e[12];
    int n = 0;
    for (int i = 0; i < 6; ++i) {
        const double p = f[2 * i] * f[2 * i + 1];
        const double t[2] = {__builtin_fma(f[2 * i], f[2 * i + 1], -p), p};
        for (int k = 0; k < 2; ++k) {
            double q = t[k];
            for (int j = 0; j < n; ++j) {
                const double s = q + e[j], bv = s - q, av = s - bv;
                e[j] = (q - av) + (e[j] - bv);
                q = s;
            }
            e[n++] = q;
        }
    }
    int sign = 0;
    for (int i = 0; i < 12; ++i) {  // the most significant non-zero component is the last one
        if (e[i] > 0.0) sign = 1;
        if (e[i] < 0.0) sign = -1;
    }
    return sign;
}
// +1: c left of a -> b (counter-clockwise), -1: right, 0: collinear
GPK_TRI_FN int orient(P2 a, P2 b, P2 c) {
    const double l = (a.x - c.x) * (b.y - c.y), r = (a.y - c.y) * (b.x - c.x), det = l - r;
    const double bound = 3.3306690738754716e-16 * (fabs(l) + fabs(r));
    const bool opposite = (l > 0.0 && r <= 0.0) || (l < 0.0 && r >= 0.0) || l == 0.0;
    if (opposite || fabs(det) >= bound) return (det > 0.0) - (det < 0.0);
    return orient_exact(a.x, a.y, b.x, b.y, c.x, c.y);
}
GPK_TRI_FN bool same(P2 a, P2 b) { return a.x == b.x && a.y == b.y; }
GPK_TRI_FN bool finite(P2 p) { return fabs(p.x) < INFINITY && fabs(p.y) < INFINITY; }  // (false for NaN)
GPK_TRI_FN bool in_box(P2 a, P2 b, P2 p) {  // the closed box of a and b
    return p.x >= fmin(a.x, b.x) && p.x <= fmax(a.x, b.x) && p.y >= fmin(a.y, b.y) && p.y <= fmax(a.y, b.y);
}
// p in the open segment ab
GPK_TRI_FN bool on_open(P2 a, P2 b, P2 p) { return in_box(a, b, p) && !same(p, a) && !same(p, b) && orient(a, b, p) == 0; }
// p on the open ray from a through b, given that a, b, p are collinear
GPK_TRI_FN bool same_way(P2 a, P2 b, P2 p) {
    if (b.x != a.x) return p.x != a.x && (b.x > a.x) == (p.x > a.x);
    return p.y != a.y && (b.y > a.y) == (p.y > a.y);
}
// p strictly inside the left cone of the corner a -> b -> c (the interior is on the left of both edges)
GPK_TRI_FN bool in_cone(P2 a, P2 b, P2 c, P2 p) {
    const int o1 = orient(a, b, p), o2 = orient(b, c, p);
    return orient(a, b, c) > 0 ? (o1 > 0 && o2 > 0) : (o1 > 0 || o2 > 0);
}
// does the edge ab rule out the bridge mv
GPK_TRI_FN bool blocks_bridge(P2 m, P2 v, P2 a, P2 b) {
    const bool a_end = same(a, m) || same(a, v), b_end = same(b, m) || same(b, v);
    if (a_end || b_end) return (a_end && !b_end && on_open(m, v, b)) || (b_end && !a_end && on_open(m, v, a));
    if (fmax(a.x, b.x) < fmin(m.x, v.x) || fmin(a.x, b.x) > fmax(m.x, v.x) || fmax(a.y, b.y) < fmin(m.y, v.y) || fmin(a.y, b.y) > fmax(m.y, v.y))
        return false;
    const int o1 = orient(m, v, a), o2 = orient(m, v, b);
    if (o1 * o2 > 0) return false;
    const int o3 = orient(a, b, m), o4 = orient(a, b, v);
    if (o3 * o4 > 0) return false;
    if (o1 * o2 < 0 && o3 * o4 < 0) return true;
    return (o1 == 0 && in_box(m, v, a)) || (o2 == 0 && in_box(m, v, b)) || (o3 == 0 && in_box(a, b, m)) || (o4 == 0 && in_box(a, b, v));
}

GPK_TRI_FN int row_share(int n_coords, int n_rings) { return n_coords + 3 * n_rings; }
GPK_TRI_FN int member_count(const RowView& r) { return r.part_off ? r.p1 - r.p0 : 1; }
GPK_TRI_FN void member_rings(const RowView& r, int m, int& r0, int& r1) {
    if (r.part_off) {
        r0 = r.part_off[r.p0 + m];
        r1 = r.part_off[r.p0 + m + 1];
    } else {
        r0 = r.s0;
        r1 = r.s1;
    }
}
GPK_TRI_FN bool member_empty(const RowView& r, int r0, int r1) { return r1 <= r0 || r.ring_off[r0 + 1] == r.ring_off[r0]; }

// is the live node b an ear.  Collective: the same b on every lane, the same answer on every lane.
template <class Ctx>
GPK_TRI_FN bool is_ear(const Nodes& nd, int nn, int b, const Ctx& cx) {
    const int a = nd.prv[b], c = nd.nxt[b];
    const P2 A = nd.xy[a], B = nd.xy[b], C = nd.xy[c];
    if (orient(A, B, C) <= 0) return false;
    if (nd.nxt[c] != a) {  // (a loop of three: the diagonal is the third edge)
        const P2 PA = nd.xy[nd.prv[a]], NC = nd.xy[nd.nxt[c]];
        if (orient(PA, A, B) > 0) {  // a convex corner at a: the diagonal a -> c must leave inside it, or along the edge to PA
            const int o = orient(PA, A, C);
            if (o < 0 || (o == 0 && !same_way(A, PA, C))) return false;
        }
        if (orient(B, C, NC) > 0) {
            const int o = orient(C, NC, A);
            if (o < 0 || (o == 0 && !same_way(C, NC, A))) return false;
        }
    }
    const double x0 = fmin(A.x, fmin(B.x, C.x)), x1 = fmax(A.x, fmax(B.x, C.x)), y0 = fmin(A.y, fmin(B.y, C.y)), y1 = fmax(A.y, fmax(B.y, C.y));
    int bad = 0;
    for (int k = cx.lane; k < nn && !bad; k += Ctx::T) {
        const int t = nd.tag[k];
        if (t >= 0 || t == T_DEAD || k == a || k == b || k == c) continue;
        const P2 p = nd.xy[k];
        if (p.x < x0 || p.x > x1 || p.y < y0 || p.y > y1) continue;
        const bool at_a = same(p, A), at_b = same(p, B), at_c = same(p, C);
        if (at_a || at_b || at_c) {  // the corner's two sides, counter-clockwise: u then w
            const P2 o = at_a ? A : (at_b ? B : C), u = at_a ? B : (at_b ? C : A), w = at_a ? C : (at_b ? A : B);
            const P2 q0 = nd.xy[nd.prv[k]], q1 = nd.xy[nd.nxt[k]];
            bad = (orient(o, u, q0) > 0 && orient(o, w, q0) < 0) || (orient(o, u, q1) > 0 && orient(o, w, q1) < 0);
        } else {
            bad = orient(A, B, p) >= 0 && orient(B, C, p) >= 0 && orient(C, A, p) >= 0;
        }
    }
    return cx.ior(bad) == 0;
}

// The whole row.  nd: cap node slots; out: 3 * cap indices.  Returns GPK_TRI_*; n_tri: the triangles written, the row's answer only with
// GPK_TRI_OK (a row that fails later has written some: the caller reports zero).
// Collective over the Ctx's lanes; the caller has checked that the row is not null.
template <class Ctx>
GPK_TRI_FN int triangulate_row(const RowView& r, const Nodes& nd, int cap, uint32_t* out, const Ctx& cx, int& n_tri) {
    n_tri = 0;
    const bool w0 = cx.lane == 0;
    int nn = 0, n_built = 0;
    // ---- 1: build
    const int nm = member_count(r);
    for (int m = 0; m < nm; ++m) {
        int r0, r1;
        member_rings(r, m, r0, r1);
        if (member_empty(r, r0, r1)) continue;
        for (int s = r0; s < r1; ++s) {
            const int c0 = r.ring_off[s], n = r.ring_off[s + 1] - c0;
            if (n == 0) continue;
            if (n < 4 || !same(r.xy[c0], r.xy[c0 + n - 1])) return GPK_TRI_FAILED;
            const int first = nn;
            const P2 f = r.xy[c0];
            P2 last = f, low = f;
            int k_low = first;
            for (int c = c0; c < c0 + n - 1; ++c) {
                const P2 p = r.xy[c];
                if (!finite(p)) return GPK_TRI_FAILED;
                if (nn > first && same(p, last)) continue;
                if (nn >= cap) return GPK_TRI_FAILED;
                if (w0) {
                    nd.xy[nn] = p;
                    nd.cix[nn] = c;
                    nd.tag[nn] = s - r.s0;
                    nd.prv[nn] = nn - 1;
                    nd.nxt[nn] = nn + 1;
                }
                if (p.x < low.x || (p.x == low.x && p.y < low.y)) low = p, k_low = nn;
                last = p;
                ++nn;
            }
            if (nn - first > 1 && same(last, f)) --nn;  // (the run before the closing coordinate)
            if (nn - first < 3) return GPK_TRI_FAILED;
            if (w0) {
                nd.prv[first] = nn - 1;
                nd.nxt[nn - 1] = first;
            }
            cx.sync();
            const int turn = orient(nd.xy[k_low == first ? nn - 1 : k_low - 1], nd.xy[k_low], nd.xy[k_low == nn - 1 ? first : k_low + 1]);
            if (turn == 0) return GPK_TRI_FAILED;
            if (turn != (s == r0 ? 1 : -1)) {
                for (int k = first + cx.lane; k < nn; k += Ctx::T) {
                    const int t = nd.prv[k];
                    nd.prv[k] = nd.nxt[k];
                    nd.nxt[k] = t;
                }
            }
            cx.sync();
            ++n_built;
        }
    }
    if (n_built == 0) return GPK_TRI_EMPTY;
    // ---- 2: split at touches
    if (n_built > 1) {
        const int n0 = nn;
        for (int w = 0; w < n0; ++w) {
            const P2 pw = nd.xy[w];
            const int tw = nd.tag[w];
            for (int guard = 0; guard < cap; ++guard) {
                int mine = NONE;
                for (int u = cx.lane; u < nn; u += Ctx::T) {
                    if (nd.tag[u] == tw) continue;
                    const P2 A = nd.xy[u], B = nd.xy[nd.nxt[u]];
                    if (on_open(A, B, pw)) {
                        mine = u;
                        break;
                    }
                }
                const int u = cx.imin(mine);
                if (u == NONE) break;
                if (nn >= cap) return GPK_TRI_FAILED;
                cx.sync();
                if (w0) {
                    const int v = nd.nxt[u];
                    nd.xy[nn] = pw;
                    nd.cix[nn] = nd.cix[w];
                    nd.tag[nn] = nd.tag[u];
                    nd.prv[nn] = u;
                    nd.nxt[nn] = v;
                    nd.prv[v] = nn;
                    nd.nxt[u] = nn;
                }
                ++nn;
                cx.sync();
            }
        }
    }
    // ---- per member: 3 merge, 4 clip, 5 spikes
    for (int m = 0; m < nm; ++m) {
        int r0, r1;
        member_rings(r, m, r0, r1);
        if (member_empty(r, r0, r1)) continue;
        const int t0 = r0 - r.s0, t1 = r1 - r.s0;
        for (int h = t0 + 1; h < t1; ++h) {  // (at most one merge a hole)
            double bx = INFINITY, by = INFINITY;
            int bk = NONE;
            for (int k = cx.lane; k < nn; k += Ctx::T) {
                const int t = nd.tag[k];
                if (t <= t0 || t >= t1) continue;
                const P2 p = nd.xy[k];
                if (p.x < bx || (p.x == bx && p.y < by)) bx = p.x, by = p.y, bk = k;
            }
            const double gx = cx.dmin(bx), gy = cx.dmin(bx == gx ? by : INFINITY);
            const int M = cx.imin(bx == gx && by == gy ? bk : NONE);
            if (M == NONE) break;  // (empty holes: fewer rings than numbers)
            const int tm = nd.tag[M], pm = nd.prv[M], nm_ = nd.nxt[M];
            const P2 PM = nd.xy[M], MP = nd.xy[pm], MN = nd.xy[nm_];
            int mine = NONE;
            for (int k = cx.lane; k < nn; k += Ctx::T) {  // a loop node at M whose cone holds the hole
                if (nd.tag[k] != t0 || !same(nd.xy[k], PM)) continue;
                const P2 a = nd.xy[nd.prv[k]], c = nd.xy[nd.nxt[k]];
                if (in_cone(a, PM, c, MP) && in_cone(a, PM, c, MN)) {
                    mine = k;
                    break;
                }
            }
            int V = cx.imin(mine);
            const bool zero = V != NONE;
            if (!zero) {
                for (int k = 0; k < nn && V == NONE; ++k) {
                    if (nd.tag[k] != t0) continue;
                    const P2 PV = nd.xy[k];
                    if (same(PV, PM)) continue;
                    if (!in_cone(nd.xy[nd.prv[k]], PV, nd.xy[nd.nxt[k]], PM) || !in_cone(MP, PM, MN, PV)) continue;
                    int bad = 0;
                    for (int u = cx.lane; u < nn && !bad; u += Ctx::T) {
                        const int t = nd.tag[u];
                        if (t < t0 || t >= t1) continue;
                        bad = blocks_bridge(PM, PV, nd.xy[u], nd.xy[nd.nxt[u]]);
                    }
                    if (cx.ior(bad) == 0) V = k;
                }
                if (V == NONE || nn + 2 > cap) return GPK_TRI_FAILED;
            }
            cx.sync();
            if (w0) {
                const int nv = nd.nxt[V];
                if (zero) {  // .. V, hole from M's next round to M, V's next ..
                    nd.nxt[V] = nm_;
                    nd.prv[nm_] = V;
                    nd.nxt[M] = nv;
                    nd.prv[nv] = M;
                } else {  // .. V, M, hole, M', V', V's next ..
                    const int M2 = nn, V2 = nn + 1;
                    nd.xy[M2] = PM, nd.cix[M2] = nd.cix[M], nd.tag[M2] = t0;
                    nd.xy[V2] = nd.xy[V], nd.cix[V2] = nd.cix[V], nd.tag[V2] = t0;
                    nd.nxt[V] = M, nd.prv[M] = V;
                    nd.nxt[pm] = M2, nd.prv[M2] = pm;
                    nd.nxt[M2] = V2, nd.prv[V2] = M2;
                    nd.nxt[V2] = nv, nd.prv[nv] = V2;
                }
            }
            if (!zero) nn += 2;
            cx.sync();
            for (int k = cx.lane; k < nn; k += Ctx::T)
                if (nd.tag[k] == tm) nd.tag[k] = t0;
            cx.sync();
        }
        for (int k = cx.lane; k < nn; k += Ctx::T)
            if (nd.tag[k] == t0) nd.tag[k] = T_LIVE;
        cx.sync();
        bool done = false, reopened = false;
        for (int it = 0; it < 4 * cap + 8 && !done; ++it) {
            int mine = NONE;
            for (int k = cx.lane; k < nn; k += Ctx::T) {
                const int t = nd.tag[k];
                if (t == T_LIVE || t == T_EAR) {
                    mine = k;
                    break;
                }
            }
            const int b = cx.imin(mine);
            if (b == NONE) {
                if (reopened) return GPK_TRI_FAILED;
                reopened = true;
                cx.sync();
                for (int k = cx.lane; k < nn; k += Ctx::T)
                    if (nd.tag[k] == T_NOT) nd.tag[k] = T_LIVE;
                cx.sync();
                continue;
            }
            if (nd.tag[b] == T_LIVE) {
                const bool e = is_ear(nd, nn, b, cx);
                cx.sync();
                if (w0) nd.tag[b] = e ? T_EAR : T_NOT;
                cx.sync();
                if (!e) continue;
            }
            const int a = nd.prv[b], c = nd.nxt[b];
            if (n_tri >= cap) return GPK_TRI_FAILED;
            if (w0) {
                out[3 * n_tri] = (uint32_t)nd.cix[a];
                out[3 * n_tri + 1] = (uint32_t)nd.cix[b];
                out[3 * n_tri + 2] = (uint32_t)nd.cix[c];
            }
            ++n_tri;
            reopened = false;
            const bool last = nd.nxt[c] == a;
            cx.sync();
            if (w0) {
                nd.tag[b] = T_DEAD;
                nd.tag[a] = nd.tag[c] = last ? T_DEAD : T_LIVE;
                nd.nxt[a] = c;
                nd.prv[c] = a;
            }
            cx.sync();
            if (last) {
                done = true;
                break;
            }
            int j = a;
            for (int guard = 0; guard < cap; ++guard) {  // spikes at the junction j -> its next
                const int p = nd.prv[j], q = nd.nxt[j], qq = nd.nxt[q];
                int x0, x1, keep0, keep1;  // remove x0, x1; keep0 -> keep1 become neighbours
                if (same(nd.xy[p], nd.xy[q])) {
                    x0 = j, x1 = q, keep0 = p, keep1 = qq;
                } else if (same(nd.xy[j], nd.xy[qq])) {
                    x0 = q, x1 = qq, keep0 = j, keep1 = nd.nxt[qq];
                } else {
                    break;
                }
                const bool gone = keep0 == x0 || keep0 == x1 || keep1 == x0 || keep1 == x1 || keep0 == keep1 || nd.nxt[keep1] == keep0;
                cx.sync();
                if (w0) {
                    nd.tag[x0] = nd.tag[x1] = T_DEAD;
                    if (gone) {  // what is left has no area
                        nd.tag[keep0] = nd.tag[keep1] = T_DEAD;
                    } else {
                        nd.tag[keep0] = nd.tag[keep1] = T_LIVE;
                        nd.nxt[keep0] = keep1;
                        nd.prv[keep1] = keep0;
                    }
                }
                cx.sync();
                if (gone) {
                    done = true;
                    break;
                }
                j = keep0;
            }
        }
        if (!done) return GPK_TRI_FAILED;
    }
    return GPK_TRI_OK;
}

}  // namespace tri
}  // namespace gpk
