// gpk_linref.h — linear referencing: WHICH segment of a geometry is nearest to a point (an arg-min scan), the nearest point on it,
// and the measure (length along the line) before it.
//   geo 0.27 ClosestPoint / LineLocatePoint / LineInterpolatePoint; shapely / GeoPandas project, interpolate, shortest_line.
// Shared by the three entry points of gpk_linref.hip.  The per-segment arithmetic and the comparison of candidates are those of the
// row-wise distance (gpk_distance.h segment_dist2 / frac_less): the winning segment is a segment at the distance `distance` returns.
// Nothing here is instantiated by the distance, nearest or dwithin kernels.
#pragma once

#include <climits>

#include "gpk_device.h"
#include "gpk_distance.h"

namespace gpk {

// ---- the arg-min accumulator -------------------------------------------------------------------------------------------------
// idx: coordinate index (in the column's coordinate buffer) of the segment's start; end: of its end (== idx for a one-coordinate
// sequence or a MULTIPOINT member: a degenerate segment).  idx == INT_MAX: no candidate yet.
// Tie rule: a candidate replaces the best only when it is strictly less (frac_less).  A lane sees its segments in ascending
// index order, so it keeps the lowest index among its ties; the cross-lane reduction takes the lower index whenever neither
// side is less.  The winner is therefore the lowest-index minimising segment, whatever the lane-group size.
struct ArgMin {
    Frac d;
    int idx, end;
};
__device__ __forceinline__ ArgMin argmin_none() { return ArgMin{Frac{INFINITY, 1.0}, INT_MAX, INT_MAX}; }

__device__ __forceinline__ void argmin_offer(ArgMin& a, const Frac& d, int idx, int end) {
    if (frac_less(d, a.d)) {
        a.d = d;
        a.idx = idx;
        a.end = end;
    }
}

template <int G>
__device__ __forceinline__ ArgMin argmin_reduce(ArgMin v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const ArgMin w{Frac{__shfl_xor(v.d.num, o, 64), __shfl_xor(v.d.den, o, 64)}, __shfl_xor(v.idx, o, 64), __shfl_xor(v.end, o, 64)};
        const bool take = frac_less(w.d, v.d) || (!frac_less(v.d, w.d) && w.idx < v.idx);
        if (take) v = w;
    }
    return v;
}

// Segments of one coordinate sequence [c0, c1) offered to the lane's accumulator (no reduction: one per row, at the end).
// POS: also the winding number and boundary flag of the sequence taken as a ring (dev::ring_edge, as scan_sequence does),
// reduced over the group; returns the ring position (POS_OUTSIDE when !POS).
template <int G, bool POS>
__device__ __forceinline__ int argmin_sequence(const double2* __restrict__ xy, int c0, int c1, double px, double py, int lane, ArgMin& a) {
    int wn = 0, on_ring = 0;
    if (c1 - c0 == 1) {
        const double2 s = xy[c0];
        if (lane == 0) {
            double cross, dxdy;
            argmin_offer(a, segment_dist2(px, py, s.x, s.y, s.x, s.y, cross, dxdy), c0, c0);
        }
        if (POS) on_ring = s.x == px && s.y == py;
    }
    for (int i = c0 + lane; i + 1 < c1; i += G) {
        const double2 s = xy[i], e = xy[i + 1];
        if (POS) {
            int w = 0;
            on_ring |= (int)dev::ring_edge(s.x, s.y, e.x, e.y, px, py, w);
            wn += w;
        }
        double cross, dxdy;
        argmin_offer(a, segment_dist2(px, py, s.x, s.y, e.x, e.y, cross, dxdy), i, i + 1);
    }
    if (!POS || c1 == c0) return dev::POS_OUTSIDE;
    if (gor<G>(on_ring)) return dev::POS_BOUNDARY;
    return gsum<G>(wn) == 0 ? dev::POS_OUTSIDE : dev::POS_INSIDE;
}

// One polygon (rings r0 .. r1, exterior first): true when the point is inside or on the boundary, by the position rules of
// point_polygon (holes excluded); else every ring's segments have been offered.  A polygon without an exterior offers nothing.
template <int G>
__device__ __forceinline__ bool argmin_polygon(const DevGeo& b, int r0, int r1, double px, double py, int lane, ArgMin& a) {
    if (r1 <= r0) return false;
    const int e0 = b.ring_off[r0], e1 = b.ring_off[r0 + 1];
    if (e1 == e0) return false;
    const int pe = argmin_sequence<G, true>(b.xy, e0, e1, px, py, lane, a);
    if (pe == dev::POS_BOUNDARY) return true;
    bool in_hole = false;
    for (int r = r0 + 1; r < r1; ++r) {
        const int ph = argmin_sequence<G, true>(b.xy, b.ring_off[r], b.ring_off[r + 1], px, py, lane, a);
        if (pe == dev::POS_INSIDE && !in_hole) {  // the first hole that is not outside decides (point_polygon's `resolved`)
            if (ph == dev::POS_BOUNDARY) return true;
            in_hole = ph == dev::POS_INSIDE;
        }
    }
    return pe == dev::POS_INSIDE && !in_hole;
}

// Row j of b: the reduced arg-min over every segment of every coordinate sequence; *inside: b is polygonal and the point is not
// outside it (the accumulator is then meaningless).
template <int G, int KIND>
__device__ __forceinline__ ArgMin argmin_row(const DevGeo& b, int64_t j, double px, double py, int lane, bool* inside) {
    ArgMin a = argmin_none();
    *inside = false;
    if (KIND == GPK_GEOM_MULTIPOINT) {
        for (int i = b.geom_off[j] + lane; i < b.geom_off[j + 1]; i += G) {
            const double2 s = b.xy[i];
            double cross, dxdy;
            argmin_offer(a, segment_dist2(px, py, s.x, s.y, s.x, s.y, cross, dxdy), i, i);
        }
    } else if (KIND == GPK_GEOM_LINESTRING) {
        argmin_sequence<G, false>(b.xy, b.geom_off[j], b.geom_off[j + 1], px, py, lane, a);
    } else if (KIND == GPK_GEOM_MULTILINESTRING) {
        for (int l = b.geom_off[j]; l < b.geom_off[j + 1]; ++l)
            argmin_sequence<G, false>(b.xy, b.ring_off[l], b.ring_off[l + 1], px, py, lane, a);
    } else {
        int p0, p1;
        dev::geom_parts(b, j, p0, p1);
        for (int p = p0; p < p1; ++p) {
            int r0, r1;
            dev::part_rings(b, p, r0, r1);
            if (argmin_polygon<G>(b, r0, r1, px, py, lane, a)) {
                *inside = true;
                return a;
            }
        }
    }
    return argmin_reduce<G>(a);
}

// ---- the nearest point of one segment ------------------------------------------------------------------------------------------
// Same differences, dot and d2 as segment_dist2, hence the same branch: q = s for a degenerate segment or dot <= 0, q = e for
// dot >= d2 (both bit for bit), else s + (dot / d2)(e - s).  *along: the length from s to q.
__device__ __forceinline__ double2 segment_nearest(double px, double py, double2 s, double2 e, double* along) {
    const double dx = e.x - s.x, dy = e.y - s.y, qx = px - s.x, qy = py - s.y;
    const double d2 = dx * dx + dy * dy;
    const double dot = qx * dx + qy * dy;
    *along = 0.0;
    if (d2 == 0.0 || dot <= 0.0) return s;
    if (dot >= d2) {
        *along = sqrt(d2);
        return e;
    }
    const double t = dot / d2;
    *along = t * sqrt(d2);
    return make_double2(s.x + t * dx, s.y + t * dy);
}

// ---- lengths -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double segment_length(double2 s, double2 e) {
    const double dx = e.x - s.x, dy = e.y - s.y;
    return sqrt(dx * dx + dy * dy);
}
template <int G>
__device__ __forceinline__ double gsum_f64(double v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // symmetric pairs: the same bits on every lane
    return v;
}
// inclusive prefix sum over the G lanes of a group (lane: index within the group)
template <int G>
__device__ __forceinline__ double gprefix_f64(double v, int lane) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const double w = __shfl_up(v, o, G);
        if (lane >= o) v += w;
    }
    return v;
}

// The lineal row j as member sequences [m0, m1) with coordinate offsets `off`: a LINESTRING is its own single member.
__device__ __forceinline__ void lineal_members(const DevGeo& b, int64_t j, const int32_t*& off, int& m0, int& m1) {
    if (b.type == GPK_GEOM_LINESTRING) {
        off = b.geom_off;
        m0 = (int)j;
        m1 = (int)j + 1;
    } else {
        off = b.ring_off;
        m0 = b.geom_off[j];
        m1 = b.geom_off[j + 1];
    }
}

// Length of the row's segments that start before coordinate `idx` (*before) and, when `all`, of every segment (*total): members
// in storage order, the gap between two members has no length.  Each lane sums its strided segments, then a group sum.
template <int G>
__device__ __forceinline__ void measure_before(const DevGeo& b, int64_t j, int idx, bool all, int lane, double* before, double* total) {
    const int32_t* off;
    int m0, m1;
    lineal_members(b, j, off, m0, m1);
    double sb = 0.0, st = 0.0;
    for (int m = m0; m < m1; ++m) {
        const int c0 = off[m], c1 = off[m + 1];
        if (!all && c0 >= idx) break;
        const int hi = all ? c1 - 1 : (c1 - 1 < idx ? c1 - 1 : idx);
        for (int i = c0 + lane; i < hi; i += G) {
            const double len = segment_length(b.xy[i], b.xy[i + 1]);
            st += len;
            sb += i < idx ? len : 0.0;
        }
    }
    *before = gsum_f64<G>(sb);
    *total = gsum_f64<G>(st);
}

// ---- rows of a tile, longest first -----------------------------------------------------------------------------------------------
// The schedule of the row-wise distance kernel: a work-group bins its tile of rows by log2(coordinate count) with a counting sort in
// LDS, then G-lane groups walk the tile in bin order.  Which group handles which row depends on atomic order, a row's result does not.
constexpr int LINREF_TILE = 2048, LINREF_BINS = 24;
__device__ __forceinline__ int row_coord_count(const DevGeo& b, int64_t j) {
    switch (b.type) {
    case GPK_GEOM_POINT: return 1;
    case GPK_GEOM_LINESTRING:
    case GPK_GEOM_MULTIPOINT: return b.geom_off[j + 1] - b.geom_off[j];
    case GPK_GEOM_POLYGON:
    case GPK_GEOM_MULTILINESTRING: return b.ring_off[b.geom_off[j + 1]] - b.ring_off[b.geom_off[j]];
    default: return b.ring_off[b.part_off[b.geom_off[j + 1]]] - b.ring_off[b.part_off[b.geom_off[j]]];
    }
}
// body(i, j, lane): row i of the left side, row j of `other` (may be out of range), called by all G lanes of a group
template <int G, typename Body>
__device__ __forceinline__ void for_rows_binned(int64_t n, const DevGeo& other, const uint32_t* __restrict__ rows, Body body) {
    __shared__ uint16_t s_perm[LINREF_TILE];
    __shared__ int s_cnt[LINREF_BINS], s_start[LINREF_BINS];
    const int tid = threadIdx.x, lane = tid & (G - 1);
    for (int64_t base = (int64_t)blockIdx.x * LINREF_TILE; base < n; base += (int64_t)gridDim.x * LINREF_TILE) {
        const int tile_rows = (int)(n - base < LINREF_TILE ? n - base : LINREF_TILE);
        if (tid < LINREF_BINS) s_cnt[tid] = 0;
        __syncthreads();
        int bin[LINREF_TILE / 256], rank[LINREF_TILE / 256];
#pragma unroll
        for (int k = 0; k < LINREF_TILE / 256; ++k) {
            const int li = k * 256 + tid;
            bin[k] = -1;
            if (li < tile_rows) {
                const int64_t i = base + li;
                const int64_t j = rows ? (int64_t)rows[i] : i;
                const int w = (uint64_t)j < (uint64_t)other.n_geoms ? row_coord_count(other, j) : 0;
                bin[k] = w <= 1 ? 0 : (32 - __clz(w - 1));
                if (bin[k] >= LINREF_BINS) bin[k] = LINREF_BINS - 1;
                rank[k] = atomicAdd(&s_cnt[bin[k]], 1);
            }
        }
        __syncthreads();
        if (tid == 0) {  // longest rows first
            int run = 0;
            for (int b = LINREF_BINS - 1; b >= 0; --b) {
                s_start[b] = run;
                run += s_cnt[b];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LINREF_TILE / 256; ++k)
            if (bin[k] >= 0) s_perm[s_start[bin[k]] + rank[k]] = (uint16_t)(k * 256 + tid);
        __syncthreads();
        for (int e = tid / G; e < tile_rows; e += 256 / G) {
            const int64_t i = base + s_perm[e];
            body(i, rows ? (int64_t)rows[i] : i, lane);
        }
        __syncthreads();
    }
}

}  // namespace gpk
