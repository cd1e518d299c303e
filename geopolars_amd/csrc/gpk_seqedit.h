// gpk_seqedit.h — edits of the coordinate sequences of a column (gpk_segmentize, gpk_remove_repeated_points, gpk_reverse,
// gpk_orient_polygons): the rule, host-callable.  Kernels and the driver: gpk_seqedit.hip.  Contract: include/geopolars_hip.h.
//
// A SEQUENCE is a run of coordinates under one entry of the innermost offsets level: a linestring, a member of a multilinestring, a
// ring.  All four operations rewrite the innermost offsets and the coordinate buffer and nothing else.  Per input coordinate c the
// kernels know last[c]: c is the last coordinate of its sequence (marked from the offsets; a run of equal offsets — empty sequences —
// marks nothing).
//   segmentize:  count[c] = last[c] ? 1 : pieces(xy[c], xy[c + 1], m) output coordinates begin at c; outpos = their exclusive scan.
//                Output e belongs to the LAST source c with outpos[c] <= e (Sources::find): a copy of xy[c] when e == outpos[c], else
//                piece j = e - outpos[c] of n = outpos[c + 1] - outpos[c] (interpolate).
//   remove_repeated_points:  keeps(first, xy[c], xy[c - 1]) with first = (c == 0 || last[c - 1]); outpos = the scan of the keep flags.
//   reverse / orient:  output e lies in the last sequence s with off[s] <= e (gt::Rows::find over the offsets themselves) and reads
//                reversed_source(off[s], off[s + 1], e) when that sequence is reversed.
//   orient:      per ring, argmin of (x, y, index) over every coordinate but the closing one (Cand, better: a total order, so any
//                reduction tree gives the same winner), then the neighbours that differ from it (turn_before, turn_after).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "gpk_geotake.h"

namespace gpk {
namespace se {

constexpr int LANES = gt::LANES;        // 256
constexpr int PER_LANE = gt::PER_LANE;  // 4
constexpr int STRIP = gt::STRIP;        // 1024 coordinates a work-group, in the count passes (input order) and the fills (output order)
constexpr int SOURCES = STRIP + 1;      // source coordinates a strip of the segmentize fill stages: see Sources
constexpr int64_t MAX_PIECES = (int64_t)1 << 31;

struct XY {
    double x, y;
};
GPK_GT_FN XY as_xy(const gt::Bits16& b) {
    XY p;
    memcpy(&p.x, &b.lo, 8);
    memcpy(&p.y, &b.hi, 8);
    return p;
}
GPK_GT_FN gt::Bits16 as_bits(double x, double y) {
    gt::Bits16 b;
    memcpy(&b.lo, &x, 8);
    memcpy(&b.hi, &y, 8);
    return b;
}
GPK_GT_FN bool finite(double v) { return v - v == 0.0; }

// ---- segmentize ----------------------------------------------------------------------------------------------------------------------
// the pieces of segment p -> q under the bound m: 1 unless len > m with len finite; a row's m that is NaN or <= 0 splits nothing
GPK_GT_FN int64_t pieces(XY p, XY q, double m) {
    if (!(m > 0.0)) return 1;
    const double dx = q.x - p.x, dy = q.y - p.y;
    const double len = sqrt(dx * dx + dy * dy);
    if (!(len > m) || !finite(len)) return 1;
    const double r = ceil(len / m);
    return r >= 2147483648.0 ? MAX_PIECES : (int64_t)r;
}
// coordinate j of n (0 < j < n) along p -> q: p + d * (j / n), these operations in this order
GPK_GT_FN XY interpolate(XY p, XY q, int64_t j, int64_t n) {
    const double dx = q.x - p.x, dy = q.y - p.y;
    const double t = (double)j / (double)n;
    XY r;
    r.x = p.x + dx * t;
    r.y = p.y + dy * t;
    return r;
}
// what begins at input coordinate c of n: the pieces of the segment c -> c + 1, or the coordinate alone at the end of its sequence
GPK_GT_FN int64_t segment_count(const gt::Bits16* xy, const uint8_t* last, int64_t c, int64_t n, double m) {
    return (last[c] || c + 1 >= n) ? 1 : pieces(as_xy(xy[c]), as_xy(xy[c + 1]), m);
}

// The sources of one strip of outputs [e0, e_end): first .. last are the source coordinates that own them, pos[k] = outpos[first + k]
// and xy[k] = coordinate first + k for k = 0 .. last - first + 1 (one past the last source: the far end of its segment and the start
// of the next source's outputs; outpos[n_coords] = the total closes the table).  Every source owns at least one output, so outpos is
// strictly increasing and at most STRIP sources begin inside a strip's STRIP outputs: with the one that began before the strip and
// the one past the last, SOURCES = STRIP + 1 entries always hold the window — there is no fallback to global memory.
struct Sources {
    const int32_t* pos;
    const gt::Bits16* xy;
    int64_t first, last;
    // the last source of [first, last] that begins at or before e
    GPK_GT_FN int64_t find(int64_t e) const {
        int64_t lo = 0, hi = last - first;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if ((int64_t)pos[mid] <= e)
                lo = mid;
            else
                hi = mid - 1;
        }
        return first + lo;
    }
    GPK_GT_FN gt::Bits16 value(int64_t e) const {
        const int64_t k = find(e) - first;
        const int64_t j = e - (int64_t)pos[k];
        if (j == 0) return xy[k];  // bit for bit
        const XY r = interpolate(as_xy(xy[k]), as_xy(xy[k + 1]), j, (int64_t)pos[k + 1] - (int64_t)pos[k]);
        return as_bits(r.x, r.y);
    }
};
// The last source of the strip of n_strips that ends before e_end, from the strip table (first_src[s]: the source of output s * STRIP):
// the next strip's first source, unless that one begins exactly with the next strip.
GPK_GT_FN int64_t strip_last_source(const int32_t* outpos, const int32_t* first_src, int64_t s, int64_t n_strips, int64_t n, int64_t e_end) {
    int64_t last = s + 1 < n_strips ? (int64_t)first_src[s + 1] : n - 1;
    if ((int64_t)outpos[last] >= e_end) --last;
    return last;
}
// element k of lane t of the strip that begins at e0: lane t takes t, t + LANES, ... (every store instruction of a wave covers 1 KiB of
// consecutive output, as gt::CoordPayload)
GPK_GT_FN int64_t lane_element(int64_t e0, int t, int k) { return e0 + (int64_t)k * LANES + t; }

// ---- remove_repeated_points ------------------------------------------------------------------------------------------------------------
// numeric comparison: -0.0 repeats 0.0, a NaN coordinate never repeats anything
GPK_GT_FN bool keeps(bool first, XY c, XY prev) { return first || !(c.x == prev.x && c.y == prev.y); }
GPK_GT_FN bool keeps_at(const gt::Bits16* xy, const uint8_t* last, int64_t c) {
    const bool first = c == 0 || last[c - 1] != 0;
    return first || keeps(false, as_xy(xy[c]), as_xy(xy[c - 1]));
}

// ---- reverse ---------------------------------------------------------------------------------------------------------------------------
// out[lo + k] = in[hi - 1 - k]
GPK_GT_FN int64_t reversed_source(int64_t lo, int64_t hi, int64_t e) { return lo + (hi - 1 - e); }
// the source of output e of a column whose sequences `rows` locates (start: the innermost offsets, one entry more than sequences);
// rev: a byte per sequence, nullptr: every sequence
GPK_GT_FN int64_t reverse_source(const gt::Rows& rows, const uint8_t* rev, int64_t e) {
    const int64_t s = rows.find(e);
    if (rev && !rev[s]) return e;
    const int64_t lo = rows.at(s), hi = rows.at(s + 1);
    return e < hi ? reversed_source(lo, hi, e) : e;  // (a coordinate past the last sequence's end belongs to none: copied)
}

// ---- orient ----------------------------------------------------------------------------------------------------------------------------
// a candidate for the ring's lexicographically smallest coordinate; i < 0: none yet.  bad: a non-finite coordinate was seen.
struct Cand {
    double x, y;
    int64_t i;
    bool bad;
};
GPK_GT_FN Cand no_cand() { return Cand{0.0, 0.0, -1, false}; }
// a is the winner of {a, b}: smaller x, then smaller y, then the lower index — symmetric: better(a, b) != better(b, a) for a.i != b.i
GPK_GT_FN bool better(const Cand& a, const Cand& b) {
    if (b.i < 0) return true;
    if (a.i < 0) return false;
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    return a.i < b.i;
}
GPK_GT_FN Cand merge(const Cand& a, const Cand& b) {
    Cand r = better(a, b) ? a : b;
    r.bad = a.bad || b.bad;
    return r;
}
// what lane `lane` of a group of `group` lanes sees of ring [lo, hi): coordinates lo + lane, lo + lane + group, ...; the closing
// coordinate hi - 1 is looked at (it may be the non-finite one) but is no candidate
GPK_GT_FN Cand lane_argmin(const gt::Bits16* xy, int64_t lo, int64_t hi, int lane, int group) {
    Cand best = no_cand();
    for (int64_t c = lo + lane; c < hi; c += group) {
        const XY p = as_xy(xy[c]);
        const bool bad = !(finite(p.x) && finite(p.y));  // (no candidate either: better() orders finite coordinates only)
        Cand one{p.x, p.y, (c < hi - 1 && !bad) ? c : -1, bad};
        best = merge(best, one);
    }
    return best;
}
GPK_GT_FN bool differs(XY a, XY b) { return !(a.x == b.x && a.y == b.y); }
// the nearest coordinate before / after v, cyclically over the ring's hi - lo coordinates, that differs from v; -1: there is none
GPK_GT_FN int64_t turn_before(const gt::Bits16* xy, int64_t lo, int64_t hi, int64_t v) {
    const XY pv = as_xy(xy[v]);
    int64_t c = v;
    for (int64_t k = 1; k < hi - lo; ++k) {
        c = c == lo ? hi - 1 : c - 1;
        if (differs(as_xy(xy[c]), pv)) return c;
    }
    return -1;
}
GPK_GT_FN int64_t turn_after(const gt::Bits16* xy, int64_t lo, int64_t hi, int64_t v) {
    const XY pv = as_xy(xy[v]);
    int64_t c = v;
    for (int64_t k = 1; k < hi - lo; ++k) {
        c = c == hi - 1 ? lo : c + 1;
        if (differs(as_xy(xy[c]), pv)) return c;
    }
    return -1;
}
// The turn of ring [lo, hi) given the reduced candidate: false when the ring is copied unchanged whatever the sign (fewer than 4
// coordinates, a non-finite coordinate, no two coordinates that differ from v); else u, v, w for the exact orientation.
GPK_GT_FN bool ring_turn(const gt::Bits16* xy, int64_t lo, int64_t hi, const Cand& best, int64_t* u, int64_t* v, int64_t* w) {
    if (hi - lo < 4 || best.bad || best.i < 0) return false;
    *v = best.i;
    *u = turn_before(xy, lo, hi, best.i);
    *w = turn_after(xy, lo, hi, best.i);
    return *u >= 0 && *w >= 0;
}
// s: the sign of orient(u, v, w), > 0 counter-clockwise.  shell: the ring is the first of its polygon.
GPK_GT_FN bool reverses(int s, bool shell, bool exterior_cw) {
    const bool want_ccw = shell != exterior_cw;
    return s != 0 && (s > 0) != want_ccw;
}

}  // namespace se
}  // namespace gpk
