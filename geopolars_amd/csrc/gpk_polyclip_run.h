// gpk_polyclip_run.h — the schedule that gpk_polygon_clip (gpk_polyclip.hip), gpk_polygon_union (gpk_polyunion.hip) and
// gpk_polygon_symdiff (gpk_polysymdiff.hip) share: the kernels and the host driver, over a rule type (pc::ClipRule, pu::UnionRule,
// ps::SymdiffRule) that gives the kept table and, where Rule::DIRECTION_BY_CLASS, the direction of a piece.  The count and fill kernels
// and the stitch kernel are instantiated per rule, so each call launches kernels that hold its own table only; the emit kernel does
// not depend on the rule, nor do the checks, the staging, the totals and the offsets kernel it shares with gpk_line_clip
// (gpk_clipcall.h).  Contract: include/geopolars_hip.h; the rules: gpk_polyclip.h, gpk_polyunion.h.
//
// Two sizes are unknown in turn — the arcs, then the rings — so the call is count -> scan -> fill twice over:
//   1. arc pass, counting (polygon_clip_arcs_kernel<G, CountSink>): G lanes per pair, G = lp::relation_group_size(a, b); walks ∂a
//      against b and ∂b against a and leaves the arcs and the arc coordinates of every pair, and whether its row is null.
//   2. exclusive scans of the two counts; their totals are read back (the FIRST wait) and size the arc scratch.
//   3. arc pass, filling (the same routine with FillSink, so both passes make bit-identical decisions): arc records — the two end
//      identities, the two direction neighbours, the coordinate range — and arc coordinates into workspace scratch.  The sink refuses
//      to write past the pair's counted share.
//   4. stitch (polygon_clip_stitch_kernel<G>): one group per pair.  The pair's arc table is copied into the group's LDS slice when it
//      has at most STITCH_LDS_ARCS_PER_LANE * G arcs and is read from global scratch when it has more; pc::stitch follows the links,
//      applies the junction rule and yields rings, signs and nesting, on the first lane of the group (the stitch is sequential).
//      Leaves parts, rings and coordinates per pair and the status.
//   5. exclusive scans of parts, rings, coordinates (and of the rows that stay); the totals are read back (the SECOND wait) and checked
//      against Arrow's i32 offsets before anything is allocated.
//   6. offsets (geom_offsets, validity, the compaction map) and emit (polygon_clip_emit_kernel<G>): part_offsets, ring_offsets and the
//      coordinates of every ring, the lanes strided over each arc, into the owned MULTIPOLYGON buffers.
// Everything else is stream-ordered.  Grids are uncapped, one group per pair, ceil(n / (256 / G)) blocks: there is no loop over pairs.
// Rows of many thousand coordinates run on the same lanes: correct and slow.
#pragma once

#include <climits>

#include "gpk_clipcall.h"
#include "gpk_common.h"
#include "gpk_device.h"
#include "gpk_polyclip.h"
#include "gpk_scan.h"

namespace gpk {

namespace {

// a pair with at most this many arcs per lane of its group is stitched from LDS (128-byte records: 64 KB a block at either group size)
constexpr int STITCH_LDS_ARCS_PER_LANE = 2;

struct CountSink {
    int arcs, coords;
    __device__ __forceinline__ void begin_arc(pc::End, pc::P2, int) { ++arcs; }
    __device__ __forceinline__ void coord(pc::P2) { ++coords; }
    __device__ __forceinline__ void end_arc(pc::End, pc::P2, int) {}
    __device__ __forceinline__ void rekey(int) {}
};

// BY_ARC (a rule with directions by class): an arc is backwards when its end says so, and has been given the key of its emitted start
template <bool BY_ARC>
struct FillSink {
    pc::Arc* arcs;  // the arc records
    double2* xy;    // the arc coordinates
    int arc, arc_end, at, at_end, base;  // base: the pair's first arc coordinate (Arc::c0 is relative to it)
    bool backwards, writer;              // writer: lane 0 of the group
    pc::Arc cur;
    __device__ __forceinline__ void begin_arc(pc::End s, pc::P2 s_nb, int key) {
        cur.s = s;
        cur.s_nb = s_nb;
        cur.key = key;
        cur.c0 = at - base;
    }
    __device__ __forceinline__ void coord(pc::P2 v) {
        if (writer && at < at_end) xy[at] = make_double2(v.x, v.y);
        ++at;
    }
    __device__ __forceinline__ void end_arc(pc::End e, pc::P2 e_nb, int flags) {
        cur.e = e;
        cur.e_nb = e_nb;
        cur.len = at - base - cur.c0;
        cur.flags = flags;
        if (BY_ARC ? (flags & pc::ARC_BACKWARDS) != 0 : backwards) {  // the ends and the directions of the emitted arc
            const pc::End t = cur.s;
            cur.s = cur.e;
            cur.e = t;
            const pc::P2 u = cur.s_nb;
            cur.s_nb = cur.e_nb;
            cur.e_nb = u;
            cur.flags |= pc::ARC_BACKWARDS;
        }
        if (at > at_end) cur.len = 0;  // (a truncated arc is refused by the stitcher)
        if (writer && arc < arc_end) arcs[arc] = cur;
        ++arc;
    }
    __device__ __forceinline__ void rekey(int key) { cur.key = key; }
};

template <int G, class Rule>
__global__ __launch_bounds__(256) void polygon_clip_count_kernel(DevGeo a, DevGeo b, const uint32_t* __restrict__ a_rows, const uint32_t* __restrict__ b_rows,
                                                                 int64_t n, int mode, int32_t* __restrict__ n_arcs, int32_t* __restrict__ n_acoords,
                                                                 uint8_t* __restrict__ valid) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t k = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (k >= n) return;  // (a whole group leaves together)
    CountSink sink{0, 0};
    const bool ok = pc::arcs_group<G, Rule>(a, row_of(a_rows, k, a.n_geoms), b, row_of(b_rows, k, b.n_geoms), mode, lane, sink);
    if (lane == 0) {
        n_arcs[k] = ok ? sink.arcs : 0;
        n_acoords[k] = ok ? sink.coords : 0;
        valid[k] = ok ? 1 : 0;
    }
}

// the two walks once more; ∂a fills forwards in both modes, ∂b backwards for the difference
template <int G, class Rule>
__global__ __launch_bounds__(256) void polygon_clip_fill_kernel(DevGeo a, DevGeo b, const uint32_t* __restrict__ a_rows, const uint32_t* __restrict__ b_rows,
                                                                int64_t n, int mode, const int32_t* __restrict__ arc_start,
                                                                const int32_t* __restrict__ acoord_start, pc::Arc* __restrict__ arcs,
                                                                double2* __restrict__ axy) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t k = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (k >= n) return;
    const int aa = arc_start[k], ae = arc_start[k + 1];
    if (ae <= aa) return;  // (group-uniform: a pair without arcs writes nothing)
    FillSink<Rule::DIRECTION_BY_CLASS> sink;
    sink.arcs = arcs;
    sink.xy = axy;
    sink.arc = aa;
    sink.arc_end = ae;
    sink.at = sink.base = acoord_start[k];
    sink.at_end = acoord_start[k + 1];
    sink.backwards = false;
    sink.writer = lane == 0;
    pc::RowRef ra, rb;
    if (!pc::row_ref<G>(a, row_of(a_rows, k, a.n_geoms), lane, ra) || !pc::row_ref<G>(b, row_of(b_rows, k, b.n_geoms), lane, rb)) return;
    const pc::P2 o = lc::local_origin(ra.box.x, ra.box.y, ra.box.z, ra.box.w, rb.box.x, rb.box.y, rb.box.z, rb.box.w);
    pc::walk_row_group<G, Rule>(a, ra, b, rb, a, b, pc::WALK_A, mode, o, lane, sink);
    sink.backwards = Rule::emitted_backwards(pc::WALK_B, mode);
    pc::walk_row_group<G, Rule>(b, rb, a, ra, a, b, pc::WALK_B, mode, o, lane, sink);
}

template <int G, bool INNERMOST, bool CROSSINGS>
__global__ __launch_bounds__(256) void polygon_clip_stitch_kernel(int64_t n, int drop, const int32_t* __restrict__ arc_start,
                                                                  const int32_t* __restrict__ acoord_start, const pc::Arc* __restrict__ arcs,
                                                                  const double2* __restrict__ axy, int32_t* __restrict__ next, int32_t* __restrict__ ring_first,
                                                                  int32_t* __restrict__ order, int32_t* __restrict__ info, uint8_t* __restrict__ valid,
                                                                  int32_t* __restrict__ n_parts, int32_t* __restrict__ n_rings, int32_t* __restrict__ n_coords,
                                                                  int32_t* __restrict__ keep, uint8_t* __restrict__ status) {
    constexpr int SLICE = STITCH_LDS_ARCS_PER_LANE * G;
    static_assert(sizeof(pc::Arc) == 128, "the LDS slice below is 64 KB, the static limit: a larger record needs fewer arcs a lane");
    __shared__ pc::Arc lds[256 * STITCH_LDS_ARCS_PER_LANE];
    const int lane = threadIdx.x & (G - 1), group = threadIdx.x / G;
    const int64_t k = (int64_t)blockIdx.x * (256 / G) + group;
    const bool active = k < n;
    const int a0 = active ? arc_start[k] : 0, na = active ? arc_start[k + 1] - a0 : 0;
    const pc::Arc* table = arcs + a0;
    if (na > 0 && na <= SLICE) {
        pc::Arc* slice = lds + group * SLICE;
        for (int i = lane; i < na; i += G) slice[i] = arcs[a0 + i];
        table = slice;
    }
    __syncthreads();  // (reached by every lane of the block: the groups past n carry no arcs)
    if (!active || lane != 0) return;
    int parts = 0, rings = 0, coords = 0, st = pc::ST_NULL;
    if (valid[k]) {
        st = pc::stitch<CROSSINGS>(table, na, (const pc::P2*)(axy + acoord_start[k]), lc::DevOrient{}, next + a0, ring_first + a0, order + a0, info + a0, parts, rings,
                        coords, INNERMOST);
        if (st == pc::ST_UNRESOLVED) valid[k] = 0;
        if (st <= pc::ST_TOUCH && parts == 0) st = pc::ST_EMPTY;
    }
    n_parts[k] = parts;
    n_rings[k] = rings;
    n_coords[k] = coords;
    keep[k] = drop ? (parts > 0 ? 1 : 0) : 1;
    status[k] = (uint8_t)st;
}

template <int G>
__global__ __launch_bounds__(256) void polygon_clip_emit_kernel(int64_t n, const int32_t* __restrict__ arc_start, const int32_t* __restrict__ acoord_start,
                                                                const pc::Arc* __restrict__ arcs, const double2* __restrict__ axy,
                                                                const int32_t* __restrict__ next, const int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ part_start, const int32_t* __restrict__ ring_start,
                                                                const int32_t* __restrict__ coord_start, int32_t* __restrict__ part_off,
                                                                int32_t* __restrict__ ring_off, double2* __restrict__ xy) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t k = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (k >= n) return;
    const int r0 = ring_start[k], nr = ring_start[k + 1] - r0;
    if (nr <= 0) return;
    const int a0 = arc_start[k], na = arc_start[k + 1] - a0;
    const pc::P2* pxy = (const pc::P2*)(axy + acoord_start[k]);
    int part = part_start[k], c = coord_start[k];
    const int part_end = part_start[k + 1], c_end = coord_start[k + 1];
    for (int j = 0; j < nr; ++j) {
        const int entry = order[a0 + j], first = entry & ~pc::ORDER_SHELL;
        if (lane == 0) {
            if ((entry & pc::ORDER_SHELL) && part < part_end) part_off[part] = r0 + j;
            ring_off[r0 + j] = c;
        }
        if (entry & pc::ORDER_SHELL) ++part;
        int a = first;
        for (int it = 0; it < na; ++it) {
            const pc::Arc A = arcs[a0 + a];
            for (int i = lane; i + 1 < A.len; i += G) {
                const pc::P2 v = pc::arc_coord(A, pxy, i);
                if (c + i < c_end) xy[c + i] = make_double2(v.x, v.y);
            }
            c += A.len - 1;
            a = next[a0 + a];
            if (a == first) break;
        }
        if (lane == 0 && c < c_end) {
            const pc::P2 v = pc::arc_coord(arcs[a0 + first], pxy, 0);
            xy[c] = make_double2(v.x, v.y);
        }
        ++c;
    }
}

// what a call is called: in error messages, and stage by stage in a profile
struct RunNames {
    const char *op, *count, *fill, *stitch, *totals, *offsets, *emit;
};

// The whole call behind both entry points.  mode_ok: the entry point knows the mode.
template <class Rule, bool INNERMOST>
int32_t polygon_clip_run(const RunNames& nm, bool mode_ok, const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows,
                         int64_t n_rows, int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status,
                         int32_t status_space, void* stream, gpk_geoarray** out) {
    GPK_TRY(clip_prologue(nm.op, ClipSide{"a_rows", "rows of a"}, ClipSide{"b_rows", "rows of b"}, mode_ok, mode, flags, out_src, n_rows, a, b, a_rows, b_rows,
                          out, [&](int32_t ta, int32_t tb) {
                              if (is_polygonal(ta) && is_polygonal(tb)) return (int32_t)GPK_OK;
                              return fail(GPK_ERR_MISMATCHED_GEOMETRY, "%s: POLYGON | MULTIPOLYGON x POLYGON | MULTIPOLYGON (found types %d, %d)", nm.op, ta, tb);
                          }));
    const bool drop = (flags & GPK_CLIP_DROP_EMPTY) != 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = n_rows, n1 = n > 0 ? n : 1;

    // ---- scratch of the first stage: per-pair counts, their scans, the scans' block totals, the totals record, staged lists
    const size_t words = (size_t)(n1 + 1), tot = (size_t)((n1 + 255) / 256 + 2);
    Scratch sc(workspace());
    int32_t *n_arcs, *n_acoords, *arc_start, *acoord_start, *n_parts, *n_rings, *n_coords, *keep, *part_start, *ring_start, *coord_start, *row_at;
    uint8_t *valid, *status;
    unsigned long long *tot_arcs, *tot_acoords, *tot_parts, *tot_rings, *tot_coords, *tot_rows, *totals_dev;
    ClipLists in;
    sc.add_n(words, n_arcs, n_acoords, arc_start, acoord_start, n_parts, n_rings, n_coords, keep, part_start, ring_start, coord_start, row_at);
    sc.add_n((size_t)n1, valid, status);
    sc.add_n(tot, tot_arcs, tot_acoords, tot_parts, tot_rings, tot_coords, tot_rows);
    sc.add(totals_dev, 64);
    clip_lists_plan(sc, a_rows, b_rows, rows_space, out_src, src_space, n, words, &in);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));

    // ---- 1, 2: count the arcs, scan, the first wait
    const int G = lp::relation_group_size(a->d, b->d);
    const int64_t at = (n + 255) / 256;
    unsigned long long totals[4] = {0, 0, 0, 0};  // arcs, arc coordinates
    if (n > 0) {
        GPK_LAUNCH_BY_G(nm.count, (polygon_clip_count_kernel<lp::LP_G_SMALL, Rule>), (polygon_clip_count_kernel<lp::LP_G_LARGE, Rule>), a->d, b->d, in.a_rows,
                        in.b_rows, n, (int)mode, n_arcs, n_acoords, valid);
        GPK_TRY(exclusive_scan_i32(n_arcs, n, arc_start, nullptr, tot_arcs, s));
        GPK_TRY(exclusive_scan_i32(n_acoords, n, acoord_start, nullptr, tot_acoords, s));
        GPK_TRY(clip_read_totals(nm.totals, tot_arcs + at, tot_acoords + at, nullptr, nullptr, totals_dev, totals, s));
    }
    if (totals[0] > (unsigned long long)INT32_MAX || totals[1] > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: the result exceeds 2^31 - 1 arcs / coordinates (Arrow i32 offsets)", nm.op);
    const int64_t total_arcs = (int64_t)totals[0], total_acoords = (int64_t)totals[1];

    // ---- 3, 4, 5: the arc scratch (a second arena: the first one's carves stay valid), fill, stitch, scan, the second wait
    Scratch sc2(workspace_aux(0));
    pc::Arc* arcs;
    double2* axy;
    int32_t *next, *ring_first, *order, *info;
    sc2.add(arcs, (size_t)(total_arcs + 1));
    sc2.add(axy, (size_t)(total_acoords + 1));
    sc2.add_n((size_t)(total_arcs + 1), next, ring_first, order, info);
    GPK_TRY(sc2.commit());
    unsigned long long sizes[4] = {0, 0, 0, 0};  // parts, rings, coordinates, rows that stay
    if (n > 0) {
        // (a record the fill pass should leave unwritten has length 0, which the stitcher refuses)
        GPK_HIP(hipMemsetAsync(arcs, 0, align256(sizeof(pc::Arc) * (size_t)(total_arcs + 1)), s));
        if (total_arcs > 0)
            GPK_LAUNCH_BY_G(nm.fill, (polygon_clip_fill_kernel<lp::LP_G_SMALL, Rule>), (polygon_clip_fill_kernel<lp::LP_G_LARGE, Rule>), a->d, b->d, in.a_rows,
                            in.b_rows, n, (int)mode, (const int32_t*)arc_start, (const int32_t*)acoord_start, arcs, axy);
        GPK_LAUNCH_BY_G(nm.stitch, (polygon_clip_stitch_kernel<lp::LP_G_SMALL, INNERMOST, Rule::DIRECTION_BY_CLASS>),
                        (polygon_clip_stitch_kernel<lp::LP_G_LARGE, INNERMOST, Rule::DIRECTION_BY_CLASS>), n, (int)drop,
                        (const int32_t*)arc_start, (const int32_t*)acoord_start, (const pc::Arc*)arcs, (const double2*)axy, next, ring_first, order, info, valid,
                        n_parts, n_rings, n_coords, keep, status);
        GPK_TRY(exclusive_scan_i32(n_parts, n, part_start, nullptr, tot_parts, s));
        GPK_TRY(exclusive_scan_i32(n_rings, n, ring_start, nullptr, tot_rings, s));
        GPK_TRY(exclusive_scan_i32(n_coords, n, coord_start, nullptr, tot_coords, s));
        GPK_TRY(exclusive_scan_i32(keep, n, row_at, nullptr, tot_rows, s));
        GPK_TRY(clip_read_totals(nm.totals, tot_parts + at, tot_rings + at, tot_coords + at, tot_rows + at, totals_dev + 8, sizes, s));
    }
    if (sizes[0] > (unsigned long long)INT32_MAX || sizes[1] > (unsigned long long)INT32_MAX || sizes[2] > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: the result exceeds 2^31 - 1 parts / rings / coordinates (Arrow i32 offsets)", nm.op);
    const int64_t n_out = (int64_t)sizes[3];
    const int32_t total_parts = (int32_t)sizes[0], total_rings = (int32_t)sizes[1], total_coords = (int32_t)sizes[2];

    // ---- the result column
    int device = 0;
    (void)hipGetDevice(&device);
    Column col(nm.op, GPK_GEOM_MULTIPOLYGON, device, s);
    GPK_TRY(col.size(n_out, total_parts, total_rings, total_coords, !drop && n > 0));

    // ---- 6: offsets, emit
    if (n > 0) {
        GPK_TRY(clip_write_offsets(nm.offsets, part_start, row_at, keep, valid, n, n_out, total_parts, total_rings, total_coords, col, in.src, s));
        if (total_rings > 0)
            GPK_LAUNCH_BY_G(nm.emit, (polygon_clip_emit_kernel<lp::LP_G_SMALL>), (polygon_clip_emit_kernel<lp::LP_G_LARGE>), n, (const int32_t*)arc_start,
                            (const int32_t*)acoord_start, (const pc::Arc*)arcs, (const double2*)axy, (const int32_t*)next, (const int32_t*)order,
                            (const int32_t*)part_start, (const int32_t*)ring_start, (const int32_t*)coord_start, col.part_off(), col.ring_off(), col.xy());
        if (in.src_staged && n_out > 0) GPK_TRY(copy_out(out_src, src_space, in.src, sizeof(int32_t) * (size_t)n_out, s));
        if (out_status) GPK_TRY(copy_out(out_status, status_space, status, (size_t)n, s));
    } else {
        GPK_TRY(col.zero_offsets());
    }
    col.release(out);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk
