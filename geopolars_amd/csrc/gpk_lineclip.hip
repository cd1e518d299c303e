// gpk_lineclip.hip — clip lines to polygons: gpk_line_clip over the group routine of gpk_lineclip.h.  Contract:
// include/geopolars_hip.h; the rule: gpk_lineclip.h.
//
// The first binary operation here whose result is a new column of unknown size: count -> scan -> fill.
//   1. count pass (line_clip_kernel<G, CountSink>): G lanes per pair, G = lp::relation_group_size(lines, polys); leaves the parts and
//      the coordinates of every pair, and whether its row is null.
//   2. exclusive scans of the two counts (and, with GPK_CLIP_DROP_EMPTY, of the rows that stay) — gpk_scan.h; their 64-bit totals are
//      gathered into one record and read back once (d2h_small / sync_small): the only synchronisation of the call.  The totals are
//      checked against Arrow's i32 offsets before anything is allocated.
//   3. clip_offsets_kernel (gpk_clipcall.h) writes geom_offsets, the validity bitmap and, under DROP_EMPTY, the compaction map and
//      out_src.  For a MULTILINESTRING column dropping a row without parts only removes an entry of geom_offsets.
//   4. fill pass (line_clip_kernel<G, FillSink>): the same routine with the other sink, so both passes make bit-identical decisions;
//      writes part offsets and coordinates at the pair's scanned positions.  The sink also refuses to write past the pair's counted
//      share, so a disagreement could only truncate a row, never write out of bounds.
// Grids are uncapped, one group per pair, ceil(n / (256 / G)) blocks: there is no loop over pairs and no second pass to get wrong.
// Rows of many thousand coordinates run on the same lanes: correct and slow.
#include <climits>

#include "gpk_clipcall.h"
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
    GPK_TRY(clip_prologue("line_clip", ClipSide{"line_rows", "line rows"}, ClipSide{"poly_rows", "polygon rows"},
                          mode == GPK_CLIP_INSIDE || mode == GPK_CLIP_OUTSIDE, mode, flags, out_src, n_rows, lines, polys, line_rows, poly_rows, out,
                          check_families));
    const bool drop = (flags & GPK_CLIP_DROP_EMPTY) != 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = n_rows, n1 = n > 0 ? n : 1;

    // ---- scratch: the per-pair counts, their scans, the scans' block totals, the totals record, staged row lists and out_src
    const size_t words = (size_t)(n1 + 1), tot = (size_t)((n1 + 255) / 256 + 2);
    Scratch sc(workspace());
    int32_t *n_parts, *n_coords, *keep, *part_start, *coord_start, *row_at;
    uint8_t* valid;
    unsigned long long *tot_parts, *tot_coords, *tot_rows, *totals_dev;
    ClipLists in;
    sc.add_n(words, n_parts, n_coords, keep, part_start, coord_start, row_at);
    sc.add(valid, (size_t)n1);
    sc.add_n(tot, tot_parts, tot_coords, tot_rows);
    sc.add(totals_dev, 32);
    clip_lists_plan(sc, line_rows, poly_rows, rows_space, out_src, src_space, n, words, &in);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));

    // ---- 1, 2: count, scan, the one read-back
    const int G = lp::relation_group_size(lines->d, polys->d);
    unsigned long long totals[4] = {0, 0, 0, 0};  // parts, coordinates, rows that stay
    if (n > 0) {
        GPK_LAUNCH_BY_G("gpk_line_clip_count", line_clip_count_kernel<lp::LP_G_SMALL>, line_clip_count_kernel<lp::LP_G_LARGE>, lines->d, polys->d, in.a_rows,
                        in.b_rows, n, (int)mode, (int)drop, n_parts, n_coords, keep, valid);
        GPK_TRY(exclusive_scan_i32(n_parts, n, part_start, nullptr, tot_parts, s));
        GPK_TRY(exclusive_scan_i32(n_coords, n, coord_start, nullptr, tot_coords, s));
        GPK_TRY(exclusive_scan_i32(keep, n, row_at, nullptr, tot_rows, s));
        const int64_t at = (n + 255) / 256;
        GPK_TRY(clip_read_totals("gpk_line_clip_totals", tot_parts + at, tot_coords + at, tot_rows + at, nullptr, totals_dev, totals, s));
    }
    if (totals[0] > (unsigned long long)INT32_MAX || totals[1] > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "line_clip: the result exceeds 2^31 - 1 parts / coordinates (Arrow i32 offsets)");
    const int64_t n_out = (int64_t)totals[2];
    const int32_t total_parts = (int32_t)totals[0], total_coords = (int32_t)totals[1];

    // ---- the result column: a MULTILINESTRING's parts are its ring level
    int device = 0;
    (void)hipGetDevice(&device);
    Column col("line_clip", GPK_GEOM_MULTILINESTRING, device, s);
    GPK_TRY(col.size(n_out, 0, total_parts, total_coords, !drop && n > 0));

    // ---- 3, 4: offsets, fill
    if (n > 0) {
        GPK_TRY(clip_write_offsets("gpk_line_clip_offsets", part_start, row_at, keep, valid, n, n_out, 0, total_parts, total_coords, col, in.src, s));
        if (total_parts > 0)
            GPK_LAUNCH_BY_G("gpk_line_clip_fill", line_clip_fill_kernel<lp::LP_G_SMALL>, line_clip_fill_kernel<lp::LP_G_LARGE>, lines->d, polys->d, in.a_rows,
                            in.b_rows, n, (int)mode, (const int32_t*)part_start, (const int32_t*)coord_start, col.ring_off(), col.xy());
        if (in.src_staged && n_out > 0) GPK_TRY(copy_out(out_src, src_space, in.src, sizeof(int32_t) * (size_t)n_out, s));
    } else {
        GPK_TRY(col.zero_offsets());
    }
    col.release(out);
    return GPK_OK;
}

