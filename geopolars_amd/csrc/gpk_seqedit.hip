// gpk_seqedit.hip — gpk_segmentize / gpk_remove_repeated_points / gpk_reverse / gpk_orient_polygons: the coordinate sequences of a column
// rewritten on the device.  Contract: include/geopolars_hip.h; the rule (piece count, interpolation, keep test, argmin, locate steps):
// gpk_seqedit.h.
//
// Every call copies the offsets levels above the innermost one and the bitmap as they are (device-to-device copies on the stream) and
// rewrites the innermost offsets and the coordinates.  POINT / MULTIPOINT columns (and non-polygonal ones under orient) are such a copy
// at every level.
//   heads     (one lane per sequence): last[c] = c is the last coordinate of its sequence.
//   segmentize / remove_repeated_points: one kernel, two passes over strips of 1024 INPUT coordinates (counted with coalesced loads,
//     scanned four consecutive counts a lane through LDS).
//     pass 0  the strip's total of the per-coordinate counts (pieces that begin there / the keep flag), 64-bit.
//     scan    of the strip totals (gpk_scan.h), then the call's one wait: the coordinate total, checked against i32 offsets before
//             anything is allocated.
//     pass 1  the counts again — from the coordinates, not from memory: recomputing costs a sqrt and a division, storing and reloading
//             them 16 bytes a coordinate — their prefix in registers, outpos[c] as one 16-byte store a lane; remove_repeated_points
//             writes its kept coordinates here (monotone addresses).
//     offsets new_off[s] = outpos[old_off[s]].
//     fill    (segmentize) in OUTPUT order: a work-group per strip of 1024 outputs stages its <= 1025 sources (outpos and coordinates)
//             in LDS, every output bisects there, copies or interpolates.
//   reverse / orient: no scan, no wait; the offsets are copied.  orient marks the shells (first ring of every polygon), then takes the
//     per-ring argmin — a group of 8 lanes a ring up to 256 coordinates, a work-group a longer one (listed by the first kernel; the list's
//     order does not reach the result; one work-group per ring that could be long, none loops) — and writes one byte a ring.  The fill works in output order like take's: a strip table (one
//     bisection a strip), the strip's offsets staged in LDS unless more than gt::WINDOW sequences end inside it.
#include <climits>

#include "gpk_column.h"
#include "gpk_common.h"
#include "gpk_device.h"
#include "gpk_scan.h"
#include "gpk_scratch.h"
#include "gpk_seqedit.h"

namespace gpk {

namespace {

constexpr int OP_SEGMENTIZE = 0, OP_DEDUP = 1;
constexpr int GROUP = 8;        // lanes a short ring
constexpr int SHORT_RING = 256;  // coordinates: longer rings go to a work-group

inline dim3 lanes_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)); }

// the offsets levels of a column, outermost first
struct Levels {
    const int32_t* off[gt::MAX_LEVELS];
    int64_t rows[gt::MAX_LEVELS];  // entries of the level, less one
    int n;
};
Levels levels_of(const DevGeo& d) {
    Levels L{{nullptr, nullptr, nullptr}, {0, 0, 0}, 0};
    if (d.type != GPK_GEOM_POINT) {
        L.off[L.n] = d.geom_off;
        L.rows[L.n++] = d.n_geoms;
    }
    if (d.type == GPK_GEOM_MULTIPOLYGON) {
        L.off[L.n] = d.part_off;
        L.rows[L.n++] = d.n_parts;
    }
    if (d.type == GPK_GEOM_POLYGON || d.type == GPK_GEOM_MULTILINESTRING || d.type == GPK_GEOM_MULTIPOLYGON) {
        L.off[L.n] = d.ring_off;
        L.rows[L.n++] = d.n_rings;
    }
    return L;
}

// first == 0: mark[off[s + 1] - 1] = 1 (the last coordinate of sequence s); first == 1: mark[off[s]] = 1 (the first ring of polygon s).
// A run of equal offsets marks nothing.
__global__ __launch_bounds__(256) void seqedit_mark_kernel(const int32_t* __restrict__ off, int64_t n, int first, int64_t n_children,
                                                           uint8_t* __restrict__ mark) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t lo = off[s], hi = off[s + 1];
    if (hi <= lo) return;
    const int64_t at = first ? lo : hi - 1;
    if (at >= 0 && at < n_children) mark[at] = 1;
}

// rowstart[r] = the first coordinate of row r, r = 0 .. n_rows: the walk down the first offset of every level
__global__ __launch_bounds__(256) void seqedit_rowstart_kernel(Levels L, int64_t n_rows, int32_t* __restrict__ rowstart) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rows) return;
    int64_t a = r;
    for (int l = 0; l < L.n; ++l) a = L.off[l][a];
    rowstart[r] = (int32_t)a;
}

// One work-group per strip of se::STRIP input coordinates.  The counts are taken with lane t at coordinates t, t + 256, ... (every load
// instruction of a wave covers 1 KiB of consecutive input) and left in LDS; then every lane scans four CONSECUTIVE counts, the prefix in
// registers.  PASS 0: strip_tot[strip] = the strip's sum.  PASS 1: strip_tot holds the exclusive scan of the sums; outpos[c] for every
// coordinate (one 16-byte store a lane), outpos[n] = the total, and for OP_DEDUP the kept coordinates at their places: the local
// positions go back through LDS to the lanes that hold the coordinates, so the stores of a wave are consecutive too.
template <int OP, int PASS>
__global__ __launch_bounds__(se::LANES) void seqedit_count_kernel(const gt::Bits16* __restrict__ xy, const uint8_t* __restrict__ last, int64_t n,
                                                                  double m, const double* __restrict__ per_row,
                                                                  const int32_t* __restrict__ rowstart, int64_t n_rows,
                                                                  unsigned long long* __restrict__ strip_tot, int32_t* __restrict__ outpos,
                                                                  gt::Bits16* __restrict__ out_xy) {
    __shared__ unsigned long long lds[se::LANES / 64 + 1];
    __shared__ __attribute__((aligned(16))) uint32_t lcnt[se::STRIP];  // a count is at most 2^31
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * se::STRIP;
#pragma unroll
    for (int k = 0; k < se::PER_LANE; ++k) {
        const int64_t c = se::lane_element(base, t, k);
        uint32_t cnt = 0;
        if (c < n) {
            if constexpr (OP == OP_SEGMENTIZE) {
                double mc = m;
                if (per_row) mc = per_row[gt::Rows{rowstart, nullptr, nullptr, 0, n_rows - 1}.find(c)];
                cnt = (uint32_t)se::segment_count(xy, last, c, n, mc);
            } else {
                cnt = se::keeps_at(xy, last, c) ? 1u : 0u;
            }
        }
        lcnt[k * se::LANES + t] = cnt;
    }
    __syncthreads();
    const uint4 q = *reinterpret_cast<const uint4*>(&lcnt[se::PER_LANE * t]);
    const uint32_t cnt[se::PER_LANE] = {q.x, q.y, q.z, q.w};
    unsigned long long tot;
    unsigned long long o = dev::block_exclusive_scan<unsigned long long, se::LANES>((unsigned long long)q.x + q.y + q.z + q.w, lds, &tot);
    if constexpr (PASS == 0) {
        if (t == 0) strip_tot[blockIdx.x] = tot;
    } else {
        const unsigned long long strip_base = strip_tot[blockIdx.x];  // (the total fits i32: the host checked it before this pass)
        const int64_t c0 = base + (int64_t)t * se::PER_LANE;
        int32_t y[se::PER_LANE];
#pragma unroll
        for (int k = 0; k < se::PER_LANE; ++k) {
            y[k] = (int32_t)(strip_base + o);
            if constexpr (OP == OP_DEDUP) lcnt[se::PER_LANE * t + k] = cnt[k] ? (uint32_t)o : 0xFFFFFFFFu;  // (every lane has read its counts: the scan synchronised)
            o += cnt[k];
        }
        if (c0 + se::PER_LANE <= n) {
            *reinterpret_cast<int4*>(outpos + c0) = make_int4(y[0], y[1], y[2], y[3]);  // (a 256-byte aligned carve, c0 a multiple of 4)
        } else {
#pragma unroll
            for (int k = 0; k < se::PER_LANE; ++k)
                if (c0 + k < n) outpos[c0 + k] = y[k];
        }
        if (c0 <= n - 1 && n - 1 < c0 + se::PER_LANE) outpos[n] = (int32_t)(strip_base + o);
        if constexpr (OP == OP_DEDUP) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < se::PER_LANE; ++k) {
                const int64_t c = se::lane_element(base, t, k);
                const uint32_t at = lcnt[k * se::LANES + t];
                if (c < n && at != 0xFFFFFFFFu) out_xy[strip_base + at] = xy[c];
            }
        }
    }
}

// new_off[s] = outpos[off[s]], s = 0 .. n_seq
__global__ __launch_bounds__(256) void seqedit_offsets_kernel(const int32_t* __restrict__ off, int64_t n_seq, const int32_t* __restrict__ outpos,
                                                              int64_t n, int32_t* __restrict__ new_off) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_seq) return;
    int64_t o = off[s];
    o = o < 0 ? 0 : (o > n ? n : o);
    new_off[s] = outpos[o];
}

// the strip table: the row (source coordinate, sequence) of every strip's first output element, one lane per strip
__global__ __launch_bounds__(256) void seqedit_strips_kernel(const int32_t* __restrict__ start, int64_t n_rows, int64_t n_strips,
                                                             int32_t* __restrict__ first_row) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_strips) first_row[s] = gt::strip_first_row(start, n_rows, s);
}

// segmentize, the fill: one work-group per strip of se::STRIP output coordinates
__global__ __launch_bounds__(se::LANES) void seqedit_segfill_kernel(const gt::Bits16* __restrict__ xy, const int32_t* __restrict__ outpos, int64_t n,
                                                                    int64_t total, const int32_t* __restrict__ first_src, int64_t n_strips,
                                                                    gt::Bits16* __restrict__ out) {
    __shared__ int32_t pos[se::SOURCES];
    __shared__ gt::Bits16 sxy[se::SOURCES];
    const int t = threadIdx.x;
    const int64_t strip = blockIdx.x, e0 = strip * se::STRIP;
    if (strip >= n_strips || e0 >= total) return;  // (block-uniform)
    const int64_t e_end = e0 + se::STRIP < total ? e0 + se::STRIP : total;
    const int64_t first = first_src[strip];
    const int64_t last = se::strip_last_source(outpos, first_src, strip, n_strips, n, e_end);
    const int64_t w = last - first + 2;  // with the one past the last source
    if (w > se::SOURCES) return;         // (cannot happen: outpos is strictly increasing — se::Sources)
    for (int64_t k = t; k < w; k += se::LANES) {
        pos[k] = outpos[first + k];
        if (first + k < n) sxy[k] = xy[first + k];
    }
    __syncthreads();
    const se::Sources src{pos, sxy, first, last};
#pragma unroll
    for (int k = 0; k < se::PER_LANE; ++k) {
        const int64_t e = se::lane_element(e0, t, k);
        if (e < e_end) out[e] = src.value(e);
    }
}

// reverse / orient, the fill: one work-group per strip of se::STRIP output coordinates; off: the innermost offsets (n_seq + 1 entries)
__global__ __launch_bounds__(se::LANES) void seqedit_revfill_kernel(const gt::Bits16* __restrict__ xy, const int32_t* __restrict__ off, int64_t n_seq,
                                                                    int64_t total, const int32_t* __restrict__ first_seq, int64_t n_strips,
                                                                    const uint8_t* __restrict__ rev, gt::Bits16* __restrict__ out) {
    __shared__ int32_t win[gt::WINDOW + 1];
    const int t = threadIdx.x;
    const int64_t strip = blockIdx.x, e0 = strip * se::STRIP;
    if (strip >= n_strips || e0 >= total) return;  // (block-uniform)
    const int64_t e_end = e0 + se::STRIP < total ? e0 + se::STRIP : total;
    gt::Rows rows = gt::strip_rows(off, n_seq, first_seq, strip, n_strips);
    const int64_t w = rows.last - rows.first + 1;
    if (w <= gt::WINDOW) {  // (block-uniform) the starts of the strip's sequences and the end of the last one
        for (int64_t k = t; k < w + 1; k += se::LANES) win[k] = off[rows.first + k];
        __syncthreads();
        rows.win = win;
    }
#pragma unroll
    for (int k = 0; k < se::PER_LANE; ++k) {
        const int64_t e = se::lane_element(e0, t, k);
        if (e < e_end) out[e] = xy[se::reverse_source(rows, rev, e)];
    }
}

// ---- orient: the argmin ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ se::Cand shuffle_xor(const se::Cand& c, int mask, int width) {
    se::Cand o;
    o.x = __shfl_xor(c.x, mask, width);
    o.y = __shfl_xor(c.y, mask, width);
    o.i = (int64_t)__shfl_xor((long long)c.i, mask, width);
    o.bad = __shfl_xor((int)c.bad, mask, width) != 0;
    return o;
}
__device__ __forceinline__ uint8_t ring_reverses(const gt::Bits16* __restrict__ xy, int64_t lo, int64_t hi, const se::Cand& best, bool shell,
                                                 bool exterior_cw) {
    int64_t u, v, w;
    if (!se::ring_turn(xy, lo, hi, best, &u, &v, &w)) return 0;
    const se::XY pu = se::as_xy(xy[u]), pv = se::as_xy(xy[v]), pw = se::as_xy(xy[w]);
    const int s = dev::orient2d(pu.x, pu.y, pv.x, pv.y, pw.x, pw.y);
    return se::reverses(s, shell, exterior_cw) ? 1 : 0;
}

// GROUP lanes a ring: rings of at most SHORT_RING coordinates are settled here, the others listed for seqedit_orient_long_kernel
__global__ __launch_bounds__(256) void seqedit_orient_short_kernel(const gt::Bits16* __restrict__ xy, const int32_t* __restrict__ ring_off, int64_t n_rings,
                                                                   const uint8_t* __restrict__ shell, int exterior_cw, uint8_t* __restrict__ rev,
                                                                   int32_t* __restrict__ long_list, unsigned int* __restrict__ n_long) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = gid / GROUP;
    const int lane = (int)(gid % GROUP);
    int64_t lo = 0, hi = 0;
    if (r < n_rings) {
        lo = ring_off[r];
        hi = ring_off[r + 1];
    }
    const bool is_long = hi - lo > SHORT_RING;
    se::Cand best = se::no_cand();
    if (!is_long) best = se::lane_argmin(xy, lo, hi, lane, GROUP);  // (hi == lo for the lanes past the last ring)
#pragma unroll
    for (int o = GROUP / 2; o > 0; o >>= 1) best = se::merge(best, shuffle_xor(best, o, GROUP));
    if (r >= n_rings || lane != 0) return;
    if (is_long) {
        long_list[atomicAdd(n_long, 1u)] = (int32_t)r;
        return;
    }
    rev[r] = ring_reverses(xy, lo, hi, best, shell[r] != 0, exterior_cw != 0);
}

// a work-group a listed ring: work-group i takes entry i of the list, and the grid has one work-group for every ring that COULD be listed
// (a listed ring has more than SHORT_RING coordinates), so no work-group loops and the ones past the list's end leave at once
__global__ __launch_bounds__(256) void seqedit_orient_long_kernel(const gt::Bits16* __restrict__ xy, const int32_t* __restrict__ ring_off,
                                                                  const uint8_t* __restrict__ shell, int exterior_cw, uint8_t* __restrict__ rev,
                                                                  const int32_t* __restrict__ long_list, const unsigned int* __restrict__ n_long) {
    __shared__ se::Cand part[4];
    const int t = threadIdx.x;
    if (blockIdx.x >= *n_long) return;  // (block-uniform)
    const int64_t r = long_list[blockIdx.x];
    const int64_t lo = ring_off[r], hi = ring_off[r + 1];
    se::Cand best = se::lane_argmin(xy, lo, hi, t, 256);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = se::merge(best, shuffle_xor(best, o, 64));
    if ((t & 63) == 0) part[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        best = se::merge(se::merge(part[0], part[1]), se::merge(part[2], part[3]));
        rev[r] = ring_reverses(xy, lo, hi, best, shell[r] != 0, exterior_cw != 0);
    }
}

// ---- the driver --------------------------------------------------------------------------------------------------------------------------
// the result column sized like the source but for its coordinates, and every level the operation does not rewrite copied into it
// (all of them when `innermost_too`)
int32_t begin_column(Column& col, const DevGeo& d, const Levels& L, int64_t n_coords_out, bool innermost_too, hipStream_t s) {
    GPK_TRY(col.size(d.n_geoms, d.n_parts, d.n_rings, n_coords_out, d.validity != nullptr));
    int32_t* dst[gt::MAX_LEVELS] = {nullptr, nullptr, nullptr};
    {
        int l = 0;
        if (col.geom_off()) dst[l++] = col.geom_off();
        if (col.part_off()) dst[l++] = col.part_off();
        if (col.ring_off()) dst[l++] = col.ring_off();
    }
    const int n_copy = innermost_too ? L.n : L.n - 1;
    for (int l = 0; l < n_copy; ++l)
        GPK_HIP(hipMemcpyAsync(dst[l], L.off[l], sizeof(int32_t) * (size_t)(L.rows[l] + 1), hipMemcpyDeviceToDevice, s));
    if (d.validity && d.n_geoms > 0)
        GPK_HIP(hipMemcpyAsync(col.validity(), d.validity, (size_t)((d.n_geoms + 7) / 8), hipMemcpyDeviceToDevice, s));
    return GPK_OK;
}
int32_t* innermost_of(Column& col) { return col.ring_off() ? col.ring_off() : col.geom_off(); }

// the column as it is: POINT / MULTIPOINT under every operation, a column without coordinates, a non-polygonal column under orient
int32_t copy_column(const char* op, const gpk_geoarray* a, hipStream_t s, gpk_geoarray** out) {
    const DevGeo& d = a->d;
    const Levels L = levels_of(d);
    int device = 0;
    (void)hipGetDevice(&device);
    Column col(op, d.type, device, s);
    if (d.n_geoms == 0) {  // (a column without rows: nothing of the source is read)
        GPK_TRY(col.size(0, 0, 0, 0, d.validity != nullptr));
        GPK_TRY(col.zero_offsets());
        col.release(out);
        return GPK_OK;
    }
    GPK_TRY(begin_column(col, d, L, d.n_coords, true, s));
    if (d.n_coords > 0) GPK_HIP(hipMemcpyAsync(col.xy(), d.xy, sizeof(double2) * (size_t)d.n_coords, hipMemcpyDeviceToDevice, s));
    col.release(out);
    return GPK_OK;
}
bool is_copy(const DevGeo& d) { return d.type == GPK_GEOM_POINT || d.type == GPK_GEOM_MULTIPOINT || d.n_coords == 0 || d.n_geoms == 0; }

// segmentize (per_row_in or the scalar m) and remove_repeated_points
template <int OP>
int32_t run_counted(const char* op, const gpk_geoarray* a, double m, const double* per_row_in, int32_t per_row_space, hipStream_t s, gpk_geoarray** out) {
    const DevGeo& d = a->d;
    if (is_copy(d)) return copy_column(op, a, s, out);
    const Levels L = levels_of(d);
    const int32_t* off = L.off[L.n - 1];
    const int64_t n_seq = L.rows[L.n - 1], n = d.n_coords, n_strips_in = (n + se::STRIP - 1) / se::STRIP;
    int device = 0;
    (void)hipGetDevice(&device);
    Column col(op, d.type, device, s);

    Scratch plan(workspace());
    uint8_t* last;
    unsigned long long *strip_tot, *record;
    int32_t *outpos, *rowstart;
    const double* per_row;
    plan.add(last, (size_t)n);
    plan.add(strip_tot, (size_t)n_strips_in + 1);
    plan.add(outpos, (size_t)n + 1);
    plan.stage_in(per_row, per_row_in, per_row_space, (size_t)d.n_geoms);
    plan.add_if(per_row_in != nullptr, rowstart, (size_t)d.n_geoms + 1);
    plan.add(record, 8);
    GPK_TRY(plan.commit());
    GPK_TRY(plan.upload(s));

    // ---- heads, pass 0, scan, the one read-back
    GPK_HIP(hipMemsetAsync(last, 0, (size_t)n, s));
    GPK_LAUNCH("gpk_seqedit_heads", seqedit_mark_kernel, lanes_grid(n_seq), dim3(256), 0, s, off, n_seq, 0, n, last);
    if (per_row) GPK_LAUNCH("gpk_seqedit_rowstart", seqedit_rowstart_kernel, lanes_grid(d.n_geoms + 1), dim3(256), 0, s, L, d.n_geoms, rowstart);
    const dim3 grid_in((unsigned)n_strips_in);
    constexpr auto pass0 = seqedit_count_kernel<OP, 0>;
    constexpr auto pass1 = seqedit_count_kernel<OP, 1>;
    GPK_LAUNCH("gpk_seqedit_count", pass0, grid_in, dim3(se::LANES), 0, s, (const gt::Bits16*)d.xy, (const uint8_t*)last, n, m, per_row,
               (const int32_t*)rowstart, d.n_geoms, strip_tot, (int32_t*)nullptr, (gt::Bits16*)nullptr);
    GPK_LAUNCH("gpk_scan_totals", scan_block_totals_kernel, dim3(1), dim3(1024), 0, s, strip_tot, n_strips_in, record, (unsigned long long*)nullptr);
    unsigned long long total_u = 0;
    GPK_HIP(d2h_small(&total_u, record, sizeof total_u, s));
    GPK_HIP(sync_small(s));
    if (total_u > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: the result has %llu coordinates, more than 2^31 - 1 (Arrow i32 offsets)", op, total_u);
    const int64_t total = (int64_t)total_u;

    // ---- the result column, pass 1, the offsets
    GPK_TRY(begin_column(col, d, L, total, false, s));
    GPK_LAUNCH("gpk_seqedit_place", pass1, grid_in, dim3(se::LANES), 0, s, (const gt::Bits16*)d.xy, (const uint8_t*)last, n, m, per_row,
               (const int32_t*)rowstart, d.n_geoms, strip_tot, outpos, OP == OP_DEDUP ? (gt::Bits16*)col.xy() : (gt::Bits16*)nullptr);
    GPK_LAUNCH("gpk_seqedit_offsets", seqedit_offsets_kernel, lanes_grid(n_seq + 1), dim3(256), 0, s, off, n_seq, (const int32_t*)outpos, n,
               innermost_of(col));

    // ---- segmentize: the fill, in output order.  The strip table is sized by the total: a second arena (the first one's carves stay valid).
    if (OP == OP_SEGMENTIZE && total > 0) {
        const int64_t n_strips = (total + se::STRIP - 1) / se::STRIP;
        int32_t* first_src;
        Scratch tables(workspace_aux(0));
        tables.add(first_src, (size_t)n_strips + 1);
        GPK_TRY(tables.commit());
        GPK_LAUNCH("gpk_seqedit_strips", seqedit_strips_kernel, lanes_grid(n_strips), dim3(256), 0, s, (const int32_t*)outpos, n, n_strips, first_src);
        GPK_LAUNCH("gpk_seqedit_segfill", seqedit_segfill_kernel, dim3((unsigned)n_strips), dim3(se::LANES), 0, s, (const gt::Bits16*)d.xy,
                   (const int32_t*)outpos, n, total, (const int32_t*)first_src, n_strips, (gt::Bits16*)col.xy());
    }
    col.release(out);
    return GPK_OK;
}

// reverse (orient == false: every sequence) and orient_polygons
int32_t run_reversed(const char* op, const gpk_geoarray* a, bool orient, int32_t exterior_cw, hipStream_t s, gpk_geoarray** out) {
    const DevGeo& d = a->d;
    if (is_copy(d) || (orient && !is_polygonal(d.type))) return copy_column(op, a, s, out);
    const Levels L = levels_of(d);
    const int32_t* off = L.off[L.n - 1];
    const int64_t n_seq = L.rows[L.n - 1], n = d.n_coords, n_strips = (n + se::STRIP - 1) / se::STRIP;
    int device = 0;
    (void)hipGetDevice(&device);
    Column col(op, d.type, device, s);

    Scratch plan(workspace());
    int32_t *first_seq, *long_list;
    uint8_t *shell, *rev;
    unsigned int* n_long;
    plan.add(first_seq, (size_t)n_strips + 1);
    plan.add_if(orient, shell, (size_t)n_seq);
    plan.add_if(orient, rev, (size_t)n_seq);
    plan.add_if(orient, long_list, (size_t)n_seq);
    plan.add_if(orient, n_long, 16);
    GPK_TRY(plan.commit());
    GPK_TRY(begin_column(col, d, L, n, true, s));

    if (orient) {
        const int32_t* poly_off = L.off[L.n - 2];  // geom_off of a POLYGON column, part_off of a MULTIPOLYGON one
        const int64_t n_polys = L.rows[L.n - 2];
        GPK_HIP(hipMemsetAsync(shell, 0, (size_t)n_seq, s));
        GPK_HIP(hipMemsetAsync(n_long, 0, 64, s));
        GPK_LAUNCH("gpk_seqedit_shells", seqedit_mark_kernel, lanes_grid(n_polys), dim3(256), 0, s, poly_off, n_polys, 1, n_seq, shell);
        GPK_LAUNCH("gpk_seqedit_argmin", seqedit_orient_short_kernel, lanes_grid(n_seq * GROUP), dim3(256), 0, s, (const gt::Bits16*)d.xy, off, n_seq,
                   (const uint8_t*)shell, exterior_cw, rev, long_list, n_long);
        const int64_t most_long = n / (SHORT_RING + 1) < n_seq ? n / (SHORT_RING + 1) : n_seq;  // rings of more than SHORT_RING coordinates
        if (most_long > 0)
            GPK_LAUNCH("gpk_seqedit_argmin_long", seqedit_orient_long_kernel, dim3((unsigned)most_long), dim3(256), 0, s,
                   (const gt::Bits16*)d.xy, off, (const uint8_t*)shell, exterior_cw, rev, (const int32_t*)long_list, (const unsigned int*)n_long);
    }
    GPK_LAUNCH("gpk_seqedit_strips", seqedit_strips_kernel, lanes_grid(n_strips), dim3(256), 0, s, off, n_seq, n_strips, first_seq);
    GPK_LAUNCH("gpk_seqedit_revfill", seqedit_revfill_kernel, dim3((unsigned)n_strips), dim3(se::LANES), 0, s, (const gt::Bits16*)d.xy, off, n_seq, n,
               (const int32_t*)first_seq, n_strips, orient ? (const uint8_t*)rev : (const uint8_t*)nullptr, (gt::Bits16*)col.xy());
    col.release(out);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" {

int32_t gpk_segmentize(const gpk_geoarray* a, double max_segment_length, const double* per_row, int32_t per_row_space, void* stream, gpk_geoarray** out) {
    if (!a || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "segmentize: NULL argument");
    if (per_row) {
        if (per_row_space != GPK_MEM_HOST && per_row_space != GPK_MEM_DEVICE)
            return fail(GPK_ERR_INVALID_ARGUMENT, "segmentize: unknown memory space %d", per_row_space);
    } else if (!(max_segment_length > 0.0)) {
        return fail(GPK_ERR_INVALID_ARGUMENT, "segmentize: max_segment_length must be > 0 (found %g)", max_segment_length);
    }
    GPK_TRY(require_device());
    gpk_geoarray* made = nullptr;
    GPK_TRY(run_counted<OP_SEGMENTIZE>("segmentize", a, max_segment_length, per_row, per_row_space, (hipStream_t)stream, &made));
    *out = made;
    return GPK_OK;
}

int32_t gpk_remove_repeated_points(const gpk_geoarray* a, double tolerance, void* stream, gpk_geoarray** out) {
    if (!a || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "remove_repeated_points: NULL argument");
    if (!(tolerance == 0.0))
        return fail(GPK_ERR_INVALID_ARGUMENT, "remove_repeated_points: only tolerance == 0 is implemented (found %g)", tolerance);
    GPK_TRY(require_device());
    gpk_geoarray* made = nullptr;
    GPK_TRY(run_counted<OP_DEDUP>("remove_repeated_points", a, 0.0, nullptr, GPK_MEM_HOST, (hipStream_t)stream, &made));
    *out = made;
    return GPK_OK;
}

int32_t gpk_reverse(const gpk_geoarray* a, void* stream, gpk_geoarray** out) {
    if (!a || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "reverse: NULL argument");
    GPK_TRY(require_device());
    gpk_geoarray* made = nullptr;
    GPK_TRY(run_reversed("reverse", a, false, 0, (hipStream_t)stream, &made));
    *out = made;
    return GPK_OK;
}

int32_t gpk_orient_polygons(const gpk_geoarray* a, int32_t exterior_cw, void* stream, gpk_geoarray** out) {
    if (!a || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "orient_polygons: NULL argument");
    if (exterior_cw != 0 && exterior_cw != 1) return fail(GPK_ERR_INVALID_ARGUMENT, "orient_polygons: exterior_cw must be 0 or 1 (found %d)", exterior_cw);
    GPK_TRY(require_device());
    gpk_geoarray* made = nullptr;
    GPK_TRY(run_reversed("orient_polygons", a, true, exterior_cw, (hipStream_t)stream, &made));
    *out = made;
    return GPK_OK;
}

}  // extern "C"
