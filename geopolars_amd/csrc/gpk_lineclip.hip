// gpk_lineclip.hip — clip lines to polygons: gpk_line_clip over the group routine of gpk_lineclip.h.  Contract:
// include/geopolars_hip.h; the rule: gpk_lineclip.h.
//
// The first binary operation here whose result is a new column of unknown size: count -> scan -> fill.
//   1. count pass (line_clip_kernel<G, CountSink>): G lanes per pair, G = lp::relation_group_size(lines, polys); leaves the parts and
//      the coordinates of every pair, and whether its row is null.
//   2. exclusive scans of the two counts (and, with GPK_CLIP_DROP_EMPTY, of the rows that stay) — gpk_scan.h; their 64-bit totals are
//      gathered into one record and read back once (d2h_small / sync_small): the only synchronisation of the call.  The totals are
//      checked against Arrow's i32 offsets before anything is allocated.
//   3. line_clip_offsets_kernel writes geom_offsets, the validity bitmap and, under DROP_EMPTY, the compaction map and out_src.  For a
//      MULTILINESTRING column dropping a row without parts only removes an entry of geom_offsets.
//   4. fill pass (line_clip_kernel<G, FillSink>): the same routine with the other sink, so both passes make bit-identical decisions;
//      writes part offsets and coordinates at the pair's scanned positions.  The sink also refuses to write past the pair's counted
//      share, so a disagreement could only truncate a row, never write out of bounds.
// Grids are uncapped, one group per pair, ceil(n / (256 / G)) blocks: there is no loop over pairs and no second pass to get wrong.
// Rows of many thousand coordinates run on the same lanes: correct and slow.
#include <climits>

#include "gpk_common.h"
#include "gpk_device.h"
#include "gpk_lineclip.h"
#include "gpk_scan.h"

namespace gpk {

namespace {

struct CountSink {
    int parts, coords;
    __device__ __forceinline__ void begin_part() { ++parts; }
    __device__ __forceinline__ void coord(lc::P2) { ++coords; }
};

struct FillSink {
    int32_t* part_off;  // the output's part offsets
    double2* xy;        // the output's coordinates
    int part, part_end, at, at_end;
    bool writer;  // lane 0 of the group
    __device__ __forceinline__ void begin_part() {
        if (writer && part < part_end) part_off[part] = at;
        ++part;
    }
    __device__ __forceinline__ void coord(lc::P2 v) {
        if (writer && at < at_end) xy[at] = make_double2(v.x, v.y);
        ++at;
    }
};

// rows[k] or k; an entry past the column's end: -1 (a null row)
__device__ __forceinline__ int64_t row_of(const uint32_t* __restrict__ rows, int64_t k, int64_t n_geoms) {
    const int64_t r = rows ? (int64_t)rows[k] : k;
    return r < n_geoms ? r : -1;
}

template <int G>
__global__ __launch_bounds__(256) void line_clip_count_kernel(DevGeo lines, DevGeo polys, const uint32_t* __restrict__ line_rows,
                                                              const uint32_t* __restrict__ poly_rows, int64_t n, int mode, int drop,
                                                              int32_t* __restrict__ n_parts, int32_t* __restrict__ n_coords,
                                                              int32_t* __restrict__ keep, uint8_t* __restrict__ valid) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t k = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (k >= n) return;  // (a whole group leaves together)
    CountSink sink{0, 0};
    const bool ok = lc::clip_group<G>(lines, row_of(line_rows, k, lines.n_geoms), polys, row_of(poly_rows, k, polys.n_geoms), mode, lane, sink);
    if (lane == 0) {
        const bool stays = drop ? ok && sink.parts > 0 : true;
        n_parts[k] = ok ? sink.parts : 0;
        n_coords[k] = ok ? sink.coords : 0;
        keep[k] = stays ? 1 : 0;
        valid[k] = ok ? 1 : 0;
    }
}

template <int G>
__global__ __launch_bounds__(256) void line_clip_fill_kernel(DevGeo lines, DevGeo polys, const uint32_t* __restrict__ line_rows,
                                                             const uint32_t* __restrict__ poly_rows, int64_t n, int mode,
                                                             const int32_t* __restrict__ part_start, const int32_t* __restrict__ coord_start,
                                                             int32_t* __restrict__ out_part_off, double2* __restrict__ out_xy) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t k = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (k >= n) return;
    const int pa = part_start[k], pe = part_start[k + 1];
    if (pe <= pa) return;  // (group-uniform: a pair without parts writes nothing)
    FillSink sink{out_part_off, out_xy, pa, pe, coord_start[k], coord_start[k + 1], lane == 0};
    (void)lc::clip_group<G>(lines, row_of(line_rows, k, lines.n_geoms), polys, row_of(poly_rows, k, polys.n_geoms), mode, lane, sink);
}

// the three 64-bit totals of the scans in one record
__global__ void line_clip_totals_kernel(const unsigned long long* __restrict__ parts, const unsigned long long* __restrict__ coords,
                                        const unsigned long long* __restrict__ rows, unsigned long long* __restrict__ out) {
    if (threadIdx.x == 0) {
        out[0] = *parts;
        out[1] = *coords;
        out[2] = *rows;
    }
}

// geom_offsets, validity and the compaction map.  row_at[k]: the output row of pair k when it stays (keep[k]).
__global__ __launch_bounds__(256) void line_clip_offsets_kernel(const int32_t* __restrict__ part_start, const int32_t* __restrict__ row_at,
                                                                const int32_t* __restrict__ keep, const uint8_t* __restrict__ valid, int64_t n,
                                                                int64_t n_out, int32_t total_parts, int32_t total_coords,
                                                                int32_t* __restrict__ geom_off, int32_t* __restrict__ part_off,
                                                                uint8_t* __restrict__ validity, int32_t* __restrict__ out_src) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) {
        geom_off[n_out] = total_parts;
        part_off[total_parts] = total_coords;
    }
    if (k < n && keep[k]) {
        const int64_t row = row_at[k];
        if (row < n_out) {
            geom_off[row] = part_start[k];
            if (out_src) out_src[row] = (int32_t)k;
        }
    }
    // (validity only without DROP_EMPTY: output row == pair; one lane per byte of the bitmap)
    if (validity && k < (n + 7) / 8) {
        unsigned bits = 0;
        for (int b = 0; b < 8; ++b)
            if (8 * k + b < n && valid[8 * k + b]) bits |= 1u << b;
        validity[k] = (uint8_t)bits;
    }
}

inline dim3 pair_grid(int64_t n, int G) { return dim3((unsigned)((n + (256 / G) - 1) / (256 / G))); }

int32_t check_families(int32_t tl, int32_t tp) {
    if (is_lineal(tl) && is_polygonal(tp)) return GPK_OK;
    if (is_polygonal(tl) && is_lineal(tp))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "line_clip: the lineal column comes first: swap the arguments (found types %d, %d)", tl, tp);
    return fail(GPK_ERR_MISMATCHED_GEOMETRY, "line_clip: LINESTRING | MULTILINESTRING x POLYGON | MULTIPOLYGON (found types %d, %d)", tl, tp);
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_line_clip(const gpk_geoarray* lines, const gpk_geoarray* polys, const uint32_t* line_rows, const uint32_t* poly_rows,
                                 int64_t n_rows, int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, void* stream,
                                 gpk_geoarray** out) {
    // (the plain arguments are looked at first: a bad mode or flag is refused whatever else is handed over)
    if (mode != GPK_CLIP_INSIDE && mode != GPK_CLIP_OUTSIDE) return fail(GPK_ERR_INVALID_ARGUMENT, "line_clip: unknown mode %d", mode);
    if (flags & ~GPK_CLIP_DROP_EMPTY) return fail(GPK_ERR_INVALID_ARGUMENT, "line_clip: unknown flag bits 0x%x", flags);
    const bool drop = (flags & GPK_CLIP_DROP_EMPTY) != 0;
    if (out_src && !drop) return fail(GPK_ERR_INVALID_ARGUMENT, "line_clip: out_src is the map of GPK_CLIP_DROP_EMPTY, which is not set");
    if (n_rows < 0 || n_rows > (int64_t)INT32_MAX) return fail(GPK_ERR_INVALID_ARGUMENT, "line_clip: %lld pairs", (long long)n_rows);
    if (!lines || !polys || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    GPK_TRY(check_families(lines->d.type, polys->d.type));
    if (!line_rows && n_rows != lines->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_clip: %lld pairs without line_rows but %lld line rows", (long long)n_rows, (long long)lines->d.n_geoms);
    if (!poly_rows && n_rows != polys->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_clip: %lld pairs without poly_rows but %lld polygon rows", (long long)n_rows, (long long)polys->d.n_geoms);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = n_rows, n1 = n > 0 ? n : 1;

    // ---- scratch: the per-pair counts, their scans, the scans' block totals, the totals record, staged row lists and out_src
    const size_t i32 = align256(sizeof(int32_t) * (size_t)(n1 + 1)), tot = align256(sizeof(unsigned long long) * (size_t)((n1 + 255) / 256 + 2));
    const bool stage_rows = rows_space != GPK_MEM_DEVICE, stage_src = out_src && src_space != GPK_MEM_DEVICE;
    GPK_TRY(workspace().begin(7 * i32 + align256((size_t)n1) + 3 * tot + 256 + (stage_rows ? 2 * i32 : 0) + (stage_src ? i32 : 0) + 512));
    Workspace& w = workspace();
    int32_t* n_parts = (int32_t*)w.take(i32);
    int32_t* n_coords = (int32_t*)w.take(i32);
    int32_t* keep = (int32_t*)w.take(i32);
    int32_t* part_start = (int32_t*)w.take(i32);
    int32_t* coord_start = (int32_t*)w.take(i32);
    int32_t* row_at = (int32_t*)w.take(i32);
    uint8_t* valid = (uint8_t*)w.take((size_t)n1);
    unsigned long long* tot_parts = (unsigned long long*)w.take(tot);
    unsigned long long* tot_coords = (unsigned long long*)w.take(tot);
    unsigned long long* tot_rows = (unsigned long long*)w.take(tot);
    unsigned long long* totals_dev = (unsigned long long*)w.take(256);
    const uint32_t *lrows = line_rows, *prows = poly_rows;
    if (stage_rows && n > 0) {
        if (line_rows) {
            uint32_t* r = (uint32_t*)w.take(i32);
            GPK_HIP(hipMemcpyAsync(r, line_rows, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, s));
            lrows = r;
        }
        if (poly_rows) {
            uint32_t* r = (uint32_t*)w.take(i32);
            GPK_HIP(hipMemcpyAsync(r, poly_rows, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, s));
            prows = r;
        }
    }
    int32_t* src_dev = stage_src ? (int32_t*)w.take(i32) : out_src;

    // ---- 1, 2: count, scan, the one read-back
    const int G = lp::relation_group_size(lines->d, polys->d);
    unsigned long long totals[3] = {0, 0, 0};
    if (n > 0) {
        if (G == lp::LP_G_SMALL)
            GPK_LAUNCH("gpk_line_clip_count", line_clip_count_kernel<lp::LP_G_SMALL>, pair_grid(n, G), dim3(256), 0, s, lines->d, polys->d, lrows, prows, n,
                       (int)mode, (int)drop, n_parts, n_coords, keep, valid);
        else
            GPK_LAUNCH("gpk_line_clip_count", line_clip_count_kernel<lp::LP_G_LARGE>, pair_grid(n, G), dim3(256), 0, s, lines->d, polys->d, lrows, prows, n,
                       (int)mode, (int)drop, n_parts, n_coords, keep, valid);
        GPK_TRY(exclusive_scan_i32(n_parts, n, part_start, nullptr, tot_parts, s));
        GPK_TRY(exclusive_scan_i32(n_coords, n, coord_start, nullptr, tot_coords, s));
        GPK_TRY(exclusive_scan_i32(keep, n, row_at, nullptr, tot_rows, s));
        const int64_t at = (n + 255) / 256;
        GPK_LAUNCH("gpk_line_clip_totals", line_clip_totals_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)(tot_parts + at),
                   (const unsigned long long*)(tot_coords + at), (const unsigned long long*)(tot_rows + at), totals_dev);
        GPK_HIP(d2h_small(totals, totals_dev, sizeof totals, s));
        GPK_HIP(sync_small(s));
    }
    if (totals[0] > (unsigned long long)INT32_MAX || totals[1] > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_clip: the result exceeds 2^31 - 1 parts / coordinates (Arrow i32 offsets)");
    const int64_t n_out = (int64_t)totals[2];
    const int32_t total_parts = (int32_t)totals[0], total_coords = (int32_t)totals[1];

    // ---- the result column: owned buffers, as gpk_geoarray_concat's
    gpk_geoarray* a = new gpk_geoarray;
    memset(a, 0, sizeof *a);
    (void)hipGetDevice(&a->device);
    a->d.type = GPK_GEOM_MULTILINESTRING;
    a->d.n_geoms = n_out;
    a->d.n_rings = total_parts;
    a->d.n_coords = total_coords;
    auto done = [&](int32_t rc) {
        if (rc != GPK_OK) {
            (void)hipStreamSynchronize(s);
            gpk_geoarray_free(a);
        } else {
            *out = a;
        }
        return rc;
    };
    auto alloc = [&](int slot, size_t bytes, const void** view) -> int32_t {
        void* p = nullptr;
        const hipError_t e = device_malloc(&p, bytes ? bytes : 8);
        if (e != hipSuccess) return fail(GPK_ERR_OOM, "line_clip: device_malloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        a->owned[slot] = p;
        *view = p;
        a->nbytes += (int64_t)bytes;
        return GPK_OK;
    };
    int32_t rc = alloc(0, sizeof(double2) * (size_t)total_coords, (const void**)&a->d.xy);
    if (rc == GPK_OK) rc = alloc(1, sizeof(int32_t) * (size_t)(n_out + 1), (const void**)&a->d.geom_off);
    if (rc == GPK_OK) rc = alloc(3, sizeof(int32_t) * (size_t)(total_parts + 1), (const void**)&a->d.ring_off);
    if (rc == GPK_OK && !drop && n > 0) rc = alloc(4, (size_t)((n + 7) / 8), (const void**)&a->d.validity);
    if (rc != GPK_OK) return done(rc);

    // ---- 3, 4: offsets, fill
    if (n == 0) {
        hipError_t e = hipMemsetAsync(a->owned[1], 0, sizeof(int32_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(a->owned[3], 0, sizeof(int32_t), s);
        return done(e == hipSuccess ? GPK_OK : fail(GPK_ERR_DEVICE, "line_clip: %s", hipGetErrorString(e)));
    }
    GPK_LAUNCH_OR(done, "gpk_line_clip_offsets", line_clip_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int32_t*)part_start,
                  (const int32_t*)row_at, (const int32_t*)keep, (const uint8_t*)valid, n, n_out, total_parts, total_coords, (int32_t*)a->owned[1],
                  (int32_t*)a->owned[3], (uint8_t*)a->owned[4], src_dev);
    if (total_parts > 0) {
        if (G == lp::LP_G_SMALL)
            GPK_LAUNCH_OR(done, "gpk_line_clip_fill", line_clip_fill_kernel<lp::LP_G_SMALL>, pair_grid(n, G), dim3(256), 0, s, lines->d, polys->d, lrows, prows,
                          n, (int)mode, (const int32_t*)part_start, (const int32_t*)coord_start, (int32_t*)a->owned[3], (double2*)a->owned[0]);
        else
            GPK_LAUNCH_OR(done, "gpk_line_clip_fill", line_clip_fill_kernel<lp::LP_G_LARGE>, pair_grid(n, G), dim3(256), 0, s, lines->d, polys->d, lrows, prows,
                          n, (int)mode, (const int32_t*)part_start, (const int32_t*)coord_start, (int32_t*)a->owned[3], (double2*)a->owned[0]);
    }
    if (stage_src && n_out > 0) {
        rc = copy_out(out_src, src_space, src_dev, sizeof(int32_t) * (size_t)n_out, s);
        if (rc != GPK_OK) return done(rc);
    }
    return done(GPK_OK);
}
