// gpk_pairdist.h — the device routines of the distance between two non-point geometries (MULTIPOINT, LINESTRING, MULTILINESTRING,
// POLYGON, MULTIPOLYGON), shared by the row-wise distance (gpk_pairdist.hip) and the within-distance join (gpk_dwithin.hip): both
// evaluate a pair with the same functions, the same lane-group size and the same lane order, so a pair has the same double in both.
// The contract of a pair and the two schedules are described in gpk_pairdist.hip.
#pragma once

#include <cfloat>

#include "gpk_device.h"
#include "gpk_distance.h"
#include "gpk_polypoly.h"

namespace gpk {

// (PD_LARGE_COST, the rows that go to the work-group schedule: gpk_frac.h)
constexpr int PD_VOTE = 32;      // walked coordinates between two group votes on "an intersection was found"
constexpr int PDL_CHUNK = 1024;  // segments of the walked side staged in LDS per round of the work-group schedule (32 KB)

// The coordinate sequences of one row.  MULTIPOINT rows have no sequence table: every coordinate is a sequence of one.
struct RowSeqs {
    const double2* xy;
    const int32_t* so;  // sequence offsets (ring_off, or geom_off for a LINESTRING row); nullptr for MULTIPOINT
    int s0, s1;         // sequences [s0, s1) of `so`
    int c0, c1;         // coordinates [c0, c1)
};
template <int KIND>
__device__ __forceinline__ RowSeqs row_seqs(const DevGeo& g, int64_t j) {
    RowSeqs r{g.xy, nullptr, 0, 0, 0, 0};
    if constexpr (KIND == GPK_GEOM_MULTIPOINT) {
        r.c0 = g.geom_off[j];
        r.c1 = g.geom_off[j + 1];
        return r;
    } else if constexpr (KIND == GPK_GEOM_LINESTRING) {
        r.so = g.geom_off;
        r.s0 = (int)j;
        r.s1 = (int)j + 1;
    } else if constexpr (KIND == GPK_GEOM_MULTIPOLYGON) {
        r.so = g.ring_off;
        r.s0 = g.part_off[g.geom_off[j]];
        r.s1 = g.part_off[g.geom_off[j + 1]];
    } else {  // POLYGON, MULTILINESTRING
        r.so = g.ring_off;
        r.s0 = g.geom_off[j];
        r.s1 = g.geom_off[j + 1];
    }
    r.c0 = r.so[r.s0];
    r.c1 = r.so[r.s1];
    return r;
}

// sequence holding coordinate c (c0 <= c < c1): the last s in [s0, s1) with so[s] <= c
__device__ __forceinline__ int seq_of(const int32_t* so, int s0, int s1, int c) {
    int lo = s0, hi = s1 - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (so[mid] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
// the end point of the segment that starts at coordinate c of sequence s (itself when c ends its sequence)
__device__ __forceinline__ double2 seg_end(const RowSeqs& r, int s, int c, double2 p) {
    return (r.so && c + 1 < r.so[s + 1]) ? r.xy[c + 1] : p;
}

// (pair_seg_dist2, the squared point-segment distance as a fraction with a Kahan cross product: gpk_frac.h)

// One segment pair: both point-segment distances (p0 against q, q0 against p) and, when the boxes meet, the exact crossing test.
struct PairAcc {
    Frac m;
    int hit;
};
__device__ __forceinline__ void pair_step(double2 p0, double2 p1, double2 q0, double2 q1, double qlx, double qhx, double qly, double qhy,
                                          PairAcc& acc) {
    const Frac d1 = pair_seg_dist2(p0.x, p0.y, q0.x, q0.y, q1.x, q1.y);
    const Frac d2 = pair_seg_dist2(q0.x, q0.y, p0.x, p0.y, p1.x, p1.y);
    if (frac_less(d1, acc.m)) acc.m = d1;
    if (frac_less(d2, acc.m)) acc.m = d2;
    if (fmax(p0.x, p1.x) < qlx || fmin(p0.x, p1.x) > qhx || fmax(p0.y, p1.y) < qly || fmin(p0.y, p1.y) > qhy) return;
    if (line_intersects_line(p0, p1, q0, q1)) acc.hit = 1;
}

// Polygon::coordinate_position with G lanes per ring (any power of two up to 64); same value on every lane of the group
template <int G>
__device__ inline int polygon_pos_lanes(const DevGeo& b, int r0, int r1, double px, double py, int lane) {
    if (r1 <= r0) return dev::POS_OUTSIDE;
    const int e0 = b.ring_off[r0], e1 = b.ring_off[r0 + 1];
    if (e1 == e0) return dev::POS_OUTSIDE;
    const int pe = pos_of(scan_sequence<G, false, true>(b.xy, e0, e1, px, py, lane), e1 - e0);
    if (pe != dev::POS_INSIDE) return pe;
    for (int r = r0 + 1; r < r1; ++r) {
        const int h0 = b.ring_off[r], h1 = b.ring_off[r + 1];
        const int ph = pos_of(scan_sequence<G, false, true>(b.xy, h0, h1, px, py, lane), h1 - h0);
        if (ph == dev::POS_BOUNDARY) return dev::POS_BOUNDARY;
        if (ph == dev::POS_INSIDE) return dev::POS_OUTSIDE;
    }
    return dev::POS_INSIDE;
}

// Does a vertex of X lie inside or on the polygonal row iy of Y?  When no segment of X meets Y's boundary, a connected sequence of X
// stays on one side of every (closed) ring of Y, so one vertex per sequence decides; MULTIPOINT members are sequences of one.  If a
// ring of Y is open or has one coordinate, every vertex is tested (invalid input only).  Test vertices first, first + stride, ...
// go to this group: the work-group schedule spreads them over its waves.
template <int G, int KY>
__device__ inline bool vertex_in_polygonal(const RowSeqs& x, const DevGeo& y, int64_t iy, int lane, int first, int stride) {
    int p0, p1, ra, rb, tmp;
    dev::geom_parts(y, iy, p0, p1);
    dev::part_rings(y, p0, ra, tmp);
    dev::part_rings(y, p1 - 1, tmp, rb);
    const bool every = !x.so || !rings_sided(y, ra, rb);
    const int n_tests = every ? x.c1 - x.c0 : x.s1 - x.s0;
    for (int t = first; t < n_tests; t += stride) {
        int c;
        if (every) {
            c = x.c0 + t;
        } else {
            c = x.so[x.s0 + t];
            if (c == x.so[x.s0 + t + 1]) continue;  // empty member
        }
        const double2 v = x.xy[c];
        for (int p = p0; p < p1; ++p) {
            int r0, r1;
            dev::part_rings(y, p, r0, r1);
            if (polygon_pos_lanes<G>(y, r0, r1, v.x, v.y, lane) != dev::POS_OUTSIDE) return true;
        }
    }
    return false;
}

// Lanes stride over the coordinates (segments) of L, the group walks every coordinate of W.  Returns the group's minimum in `acc`
// (same on every lane) or acc.hit != 0 as soon as some lane found a crossing.
template <int G>
__device__ inline void sweep_group(const RowSeqs& w, const RowSeqs& l, int lane, PairAcc& acc) {
    const int rounds = (l.c1 - l.c0 + G - 1) / G;
    int ls = l.s0;  // this lane's sequence cursor in L
    for (int k = 0; k < rounds; ++k) {
        const int c = l.c0 + k * G + lane;
        const bool active = c < l.c1;
        double2 q0 = make_double2(0.0, 0.0), q1 = q0;
        if (active) {
            q0 = l.xy[c];
            if (l.so) {
                while (l.so[ls + 1] <= c) ++ls;
            }
            q1 = seg_end(l, ls, c, q0);
        }
        const double qlx = fmin(q0.x, q1.x), qhx = fmax(q0.x, q1.x), qly = fmin(q0.y, q1.y), qhy = fmax(q0.y, q1.y);
        int ws = w.s0, wend = w.so ? w.so[w.s0 + 1] : 0;  // the walk's sequence cursor (group-uniform)
        double2 p0 = w.xy[w.c0];
        for (int i = w.c0; i < w.c1; ++i) {
            const double2 nx = i + 1 < w.c1 ? w.xy[i + 1] : p0;
            if (w.so) {
                while (wend <= i) wend = w.so[++ws + 1];
            }
            const double2 p1 = (w.so && i + 1 < wend) ? nx : p0;
            if (active) pair_step(p0, p1, q0, q1, qlx, qhx, qly, qhy, acc);
            p0 = nx;
            if ((i - w.c0) % PD_VOTE == PD_VOTE - 1) {
                acc.hit = gor<G>(acc.hit);
                if (acc.hit) return;
            }
        }
        acc.hit = gor<G>(acc.hit);
        if (acc.hit) return;
    }
    acc.m = gmin_frac<G>(acc.m);
}

// the reported distance of a disjoint pair: a computed zero (the products cancelled below one rounding) is reported as the smallest
// positive double — within the a-priori bound of the exact distance, and non-zero as the contract asks
__device__ __forceinline__ double disjoint_distance(const Frac& m) {
    const double d = frac_sqrt(m);
    return d == 0.0 ? DBL_TRUE_MIN : d;
}

// The distance of rows (ia, ib) of the canonically ordered columns (KA <= KB), G lanes on the pair; both rows valid with at least one
// coordinate each (a: row ia's sequences, b: row ib's).  Same value on every lane of the group.
template <int G, int KA, int KB>
__device__ __forceinline__ double pair_distance_group(const DevGeo& ga, int64_t ia, const RowSeqs& a, const DevGeo& gb, int64_t ib, const RowSeqs& b,
                                                      int lane) {
    bool hit = false;
    if constexpr (KB == GPK_GEOM_POLYGON || KB == GPK_GEOM_MULTIPOLYGON) hit = vertex_in_polygonal<G, KB>(a, gb, ib, lane, 0, 1);
    if constexpr (KA == GPK_GEOM_POLYGON || KA == GPK_GEOM_MULTIPOLYGON) {
        if (!hit) hit = vertex_in_polygonal<G, KA>(b, ga, ia, lane, 0, 1);
    }
    PairAcc acc{Frac{INFINITY, 1.0}, 0};
    if (!hit) {
        if (b.c1 - b.c0 >= a.c1 - a.c0)
            sweep_group<G>(a, b, lane, acc);
        else
            sweep_group<G>(b, a, lane, acc);
        hit = acc.hit != 0;
    }
    return hit ? 0.0 : disjoint_distance(acc.m);
}

// The same pair by a whole 256-lane work-group (rows above PD_LARGE_COST).  The shorter side is staged in LDS, PDL_CHUNK segments at a
// time; thread t owns coordinates t, t + 256, ... of the longer side and walks the staged chunk (broadcast reads).  The work-group votes
// after every chunk.  The result is valid on thread 0; the call ends with a barrier, so the LDS can be reused at once.
struct PairLargeLds {
    double4 seg[PDL_CHUNK];
    double num[4], den[4];
};
template <int KA, int KB>
__device__ __forceinline__ double pair_distance_workgroup(const DevGeo& ga, int64_t ia, const DevGeo& gb, int64_t ib, PairLargeLds& lds) {
    const int tid = threadIdx.x, wave = tid >> 6, lane64 = tid & 63;
    const RowSeqs a = row_seqs<KA>(ga, ia), b = row_seqs<KB>(gb, ib);
    // containment: the test vertices are spread over the four waves
    bool hit = false;
    if constexpr (KB == GPK_GEOM_POLYGON || KB == GPK_GEOM_MULTIPOLYGON) hit = vertex_in_polygonal<64, KB>(a, gb, ib, lane64, wave, 4);
    if constexpr (KA == GPK_GEOM_POLYGON || KA == GPK_GEOM_MULTIPOLYGON) {
        if (!hit) hit = vertex_in_polygonal<64, KA>(b, ga, ia, lane64, wave, 4);
    }
    hit = __syncthreads_or(hit) != 0;
    PairAcc acc{Frac{INFINITY, 1.0}, 0};
    if (!hit) {
        const bool a_walks = a.c1 - a.c0 <= b.c1 - b.c0;
        const RowSeqs& w = a_walks ? a : b;
        const RowSeqs& l = a_walks ? b : a;
        const int nw = w.c1 - w.c0;
        const int rounds = (l.c1 - l.c0 + 255) / 256;
        for (int ch = 0; ch < nw && !hit; ch += PDL_CHUNK) {
            const int len = nw - ch < PDL_CHUNK ? nw - ch : PDL_CHUNK;
            __syncthreads();  // the previous chunk is no longer read
            for (int t = tid; t < len; t += 256) {
                const int c = w.c0 + ch + t;
                const double2 p0 = w.xy[c];
                const double2 p1 = w.so ? seg_end(w, seq_of(w.so, w.s0, w.s1, c), c, p0) : p0;
                lds.seg[t] = make_double4(p0.x, p0.y, p1.x, p1.y);
            }
            __syncthreads();
            for (int k = 0; k < rounds && !hit; ++k) {
                const int c = l.c0 + k * 256 + tid;
                if (c < l.c1) {
                    const double2 q0 = l.xy[c];
                    const double2 q1 = l.so ? seg_end(l, seq_of(l.so, l.s0, l.s1, c), c, q0) : q0;
                    const double qlx = fmin(q0.x, q1.x), qhx = fmax(q0.x, q1.x), qly = fmin(q0.y, q1.y), qhy = fmax(q0.y, q1.y);
                    for (int t = 0; t < len; ++t) {
                        const double4 s = lds.seg[t];
                        pair_step(make_double2(s.x, s.y), make_double2(s.z, s.w), q0, q1, qlx, qhx, qly, qhy, acc);
                    }
                }
                hit = __syncthreads_or(acc.hit) != 0;
            }
        }
    }
    double d = 0.0;
    if (!hit) {  // the work-group minimum, waves folded in a fixed order
        const Frac m = gmin_frac<64>(acc.m);
        if (lane64 == 0) {
            lds.num[wave] = m.num;
            lds.den[wave] = m.den;
        }
        __syncthreads();
        if (tid == 0) {
            Frac best{lds.num[0], lds.den[0]};
            for (int w = 1; w < 4; ++w) {
                const Frac f{lds.num[w], lds.den[w]};
                if (frac_less(f, best)) best = f;
            }
            d = disjoint_distance(best);
        }
    }
    __syncthreads();  // LDS is reused by the next pair
    return d;
}

// lanes per row: the longer side's mean coordinate count, about four coordinates per lane, rounded to the instantiated sizes 8 / 32
static inline int pairdist_group_size(const DevGeo& a, const DevGeo& b) {
    auto mean = [](const DevGeo& g) { return g.n_geoms > 0 ? (double)g.n_coords / (double)g.n_geoms : 0.0; };
    const double m = mean(a) > mean(b) ? mean(a) : mean(b);
    return m >= 128.0 ? 32 : 8;
}

}  // namespace gpk
