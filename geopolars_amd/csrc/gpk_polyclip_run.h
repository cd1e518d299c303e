// gpk_polyclip_run.h — the schedule that gpk_polygon_clip (gpk_polyclip.hip) and gpk_polygon_union (gpk_polyunion.hip) share: the
// kernels and the host driver, over a rule type (pc::ClipRule, pu::UnionRule) that gives the kept table.  The count and fill kernels
// and the stitch kernel are instantiated per rule, so each call launches kernels that hold its own table only; the totals, offsets
// and emit kernels do not depend on the rule.  Contract: include/geopolars_hip.h; the rules: gpk_polyclip.h, gpk_polyunion.h.
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

#include "gpk_common.h"
#include "gpk_device.h"
#include "gpk_polyclip.h"
#include "gpk_scan.h"

namespace gpk {

namespace {

// a pair with at most this many arcs per lane of its group is stitched from LDS (96-byte records: 48 KB a block at either group size)
constexpr int STITCH_LDS_ARCS_PER_LANE = 2;

struct CountSink {
    int arcs, coords;
    __device__ __forceinline__ void begin_arc(pc::End, pc::P2, int) { ++arcs; }
    __device__ __forceinline__ void coord(pc::P2) { ++coords; }
    __device__ __forceinline__ void end_arc(pc::End, pc::P2, int) {}
};

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
        if (backwards) {  // the ends and the directions of the emitted arc
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
};

__device__ __forceinline__ int64_t row_of(const uint32_t* __restrict__ rows, int64_t k, int64_t n_geoms) {
    const int64_t r = rows ? (int64_t)rows[k] : k;
    return r < n_geoms ? r : -1;
}

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
    FillSink sink;
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

template <int G, bool INNERMOST>
__global__ __launch_bounds__(256) void polygon_clip_stitch_kernel(int64_t n, int drop, const int32_t* __restrict__ arc_start,
                                                                  const int32_t* __restrict__ acoord_start, const pc::Arc* __restrict__ arcs,
                                                                  const double2* __restrict__ axy, int32_t* __restrict__ next, int32_t* __restrict__ ring_first,
                                                                  int32_t* __restrict__ order, int32_t* __restrict__ info, uint8_t* __restrict__ valid,
                                                                  int32_t* __restrict__ n_parts, int32_t* __restrict__ n_rings, int32_t* __restrict__ n_coords,
                                                                  int32_t* __restrict__ keep, uint8_t* __restrict__ status) {
    constexpr int SLICE = STITCH_LDS_ARCS_PER_LANE * G;
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
        st = pc::stitch(table, na, (const pc::P2*)(axy + acoord_start[k]), lc::DevOrient{}, next + a0, ring_first + a0, order + a0, info + a0, parts, rings,
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

__global__ void polygon_clip_totals_kernel(const unsigned long long* __restrict__ t0, const unsigned long long* __restrict__ t1,
                                           const unsigned long long* __restrict__ t2, const unsigned long long* __restrict__ t3,
                                           unsigned long long* __restrict__ out) {
    if (threadIdx.x == 0) {
        out[0] = *t0;
        out[1] = *t1;
        out[2] = t2 ? *t2 : 0;
        out[3] = t3 ? *t3 : 0;
    }
}

// geom_offsets, validity and the compaction map.  row_at[k]: the output row of pair k when it stays (keep[k]).
__global__ __launch_bounds__(256) void polygon_clip_offsets_kernel(const int32_t* __restrict__ part_start, const int32_t* __restrict__ row_at,
                                                                   const int32_t* __restrict__ keep, const uint8_t* __restrict__ valid, int64_t n,
                                                                   int64_t n_out, int32_t total_parts, int32_t total_rings, int32_t total_coords,
                                                                   int32_t* __restrict__ geom_off, int32_t* __restrict__ part_off,
                                                                   int32_t* __restrict__ ring_off, uint8_t* __restrict__ validity,
                                                                   int32_t* __restrict__ out_src) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) {
        geom_off[n_out] = total_parts;
        part_off[total_parts] = total_rings;
        ring_off[total_rings] = total_coords;
    }
    if (k < n && keep[k]) {
        const int64_t row = row_at[k];
        if (row < n_out) {
            geom_off[row] = part_start[k];
            if (out_src) out_src[row] = (int32_t)k;
        }
    }
    if (validity && k < (n + 7) / 8) {
        unsigned bits = 0;
        for (int b = 0; b < 8; ++b)
            if (8 * k + b < n && valid[8 * k + b]) bits |= 1u << b;
        validity[k] = (uint8_t)bits;
    }
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

inline dim3 pair_grid(int64_t n, int G) { return dim3((unsigned)((n + (256 / G) - 1) / (256 / G))); }

// what a call is called: in error messages, and stage by stage in a profile
struct RunNames {
    const char *op, *count, *fill, *stitch, *totals, *offsets, *emit;
};

// the kernel at the pairs' group size: small and large are its instantiations for lp::LP_G_SMALL and lp::LP_G_LARGE, each in parentheses
#define GPK_PCLIP_BY_G(on_fail, name, small, large, ...)                                        \
    do {                                                                                       \
        if (G == lp::LP_G_SMALL)                                                               \
            GPK_LAUNCH_OR(on_fail, name, small, pair_grid(n, G), dim3(256), 0, s, __VA_ARGS__); \
        else                                                                                   \
            GPK_LAUNCH_OR(on_fail, name, large, pair_grid(n, G), dim3(256), 0, s, __VA_ARGS__); \
    } while (0)

// The whole call behind both entry points.  mode_ok: the entry point knows the mode.
template <class Rule, bool INNERMOST>
int32_t polygon_clip_run(const RunNames& nm, bool mode_ok, const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows,
                         int64_t n_rows, int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status,
                         int32_t status_space, void* stream, gpk_geoarray** out) {
    // (the plain arguments are looked at first, in the order of gpk_line_clip)
    if (!mode_ok) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: unknown mode %d", nm.op, mode);
    if (flags & ~GPK_CLIP_DROP_EMPTY) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", nm.op, flags);
    const bool drop = (flags & GPK_CLIP_DROP_EMPTY) != 0;
    if (out_src && !drop) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: out_src is the map of GPK_CLIP_DROP_EMPTY, which is not set", nm.op);
    if (n_rows < 0 || n_rows > (int64_t)INT32_MAX) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: %lld pairs", nm.op, (long long)n_rows);
    if (!a || !b || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!is_polygonal(a->d.type) || !is_polygonal(b->d.type))
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "%s: POLYGON | MULTIPOLYGON x POLYGON | MULTIPOLYGON (found types %d, %d)", nm.op, a->d.type, b->d.type);
    if (!a_rows && n_rows != a->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: %lld pairs without a_rows but %lld rows of a", nm.op, (long long)n_rows, (long long)a->d.n_geoms);
    if (!b_rows && n_rows != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: %lld pairs without b_rows but %lld rows of b", nm.op, (long long)n_rows, (long long)b->d.n_geoms);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = n_rows, n1 = n > 0 ? n : 1;
    auto plain = [](int32_t rc) { return rc; };

    // ---- scratch of the first stage: per-pair counts, their scans, the scans' block totals, the totals record, staged lists
    const size_t i32 = align256(sizeof(int32_t) * (size_t)(n1 + 1)), tot = align256(sizeof(unsigned long long) * (size_t)((n1 + 255) / 256 + 2));
    const bool stage_rows = rows_space != GPK_MEM_DEVICE, stage_src = out_src && src_space != GPK_MEM_DEVICE;
    GPK_TRY(workspace().begin(13 * i32 + 2 * align256((size_t)n1) + 6 * tot + 512 + (stage_rows ? 2 * i32 : 0) + (stage_src ? i32 : 0) + 512));
    Workspace& w = workspace();
    int32_t* n_arcs = (int32_t*)w.take(i32);
    int32_t* n_acoords = (int32_t*)w.take(i32);
    int32_t* arc_start = (int32_t*)w.take(i32);
    int32_t* acoord_start = (int32_t*)w.take(i32);
    int32_t* n_parts = (int32_t*)w.take(i32);
    int32_t* n_rings = (int32_t*)w.take(i32);
    int32_t* n_coords = (int32_t*)w.take(i32);
    int32_t* keep = (int32_t*)w.take(i32);
    int32_t* part_start = (int32_t*)w.take(i32);
    int32_t* ring_start = (int32_t*)w.take(i32);
    int32_t* coord_start = (int32_t*)w.take(i32);
    int32_t* row_at = (int32_t*)w.take(i32);
    uint8_t* valid = (uint8_t*)w.take((size_t)n1);
    uint8_t* status = (uint8_t*)w.take((size_t)n1);
    unsigned long long* tot_arcs = (unsigned long long*)w.take(tot);
    unsigned long long* tot_acoords = (unsigned long long*)w.take(tot);
    unsigned long long* tot_parts = (unsigned long long*)w.take(tot);
    unsigned long long* tot_rings = (unsigned long long*)w.take(tot);
    unsigned long long* tot_coords = (unsigned long long*)w.take(tot);
    unsigned long long* tot_rows = (unsigned long long*)w.take(tot);
    unsigned long long* totals_dev = (unsigned long long*)w.take(512);
    const uint32_t *arows = a_rows, *brows = b_rows;
    if (stage_rows && n > 0) {
        if (a_rows) {
            uint32_t* r = (uint32_t*)w.take(i32);
            GPK_HIP(hipMemcpyAsync(r, a_rows, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, s));
            arows = r;
        }
        if (b_rows) {
            uint32_t* r = (uint32_t*)w.take(i32);
            GPK_HIP(hipMemcpyAsync(r, b_rows, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, s));
            brows = r;
        }
    }
    int32_t* src_dev = stage_src ? (int32_t*)w.take(i32) : out_src;

    // ---- 1, 2: count the arcs, scan, the first wait
    const int G = lp::relation_group_size(a->d, b->d);
    const int64_t at = (n + 255) / 256;
    unsigned long long totals[4] = {0, 0, 0, 0};
    if (n > 0) {
        GPK_PCLIP_BY_G(plain, nm.count, (polygon_clip_count_kernel<lp::LP_G_SMALL, Rule>), (polygon_clip_count_kernel<lp::LP_G_LARGE, Rule>), a->d, b->d, arows, brows, n, (int)mode, n_arcs, n_acoords, valid);
        GPK_TRY(exclusive_scan_i32(n_arcs, n, arc_start, nullptr, tot_arcs, s));
        GPK_TRY(exclusive_scan_i32(n_acoords, n, acoord_start, nullptr, tot_acoords, s));
        GPK_LAUNCH(nm.totals, polygon_clip_totals_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)(tot_arcs + at),
                   (const unsigned long long*)(tot_acoords + at), (const unsigned long long*)nullptr, (const unsigned long long*)nullptr, totals_dev);
        GPK_HIP(d2h_small(totals, totals_dev, sizeof totals, s));
        GPK_HIP(sync_small(s));
    }
    if (totals[0] > (unsigned long long)INT32_MAX || totals[1] > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: the result exceeds 2^31 - 1 arcs / coordinates (Arrow i32 offsets)", nm.op);
    const int64_t total_arcs = (int64_t)totals[0], total_acoords = (int64_t)totals[1];

    // ---- 3, 4, 5: the arc scratch (a second arena: the first one's carves stay valid), fill, stitch, scan, the second wait
    const size_t arcs_b = align256(sizeof(pc::Arc) * (size_t)(total_arcs + 1)), axy_b = align256(sizeof(double2) * (size_t)(total_acoords + 1)),
                 link_b = align256(sizeof(int32_t) * (size_t)(total_arcs + 1));
    Workspace& w2 = workspace_aux(0);
    GPK_TRY(w2.begin(arcs_b + axy_b + 4 * link_b + 256));
    pc::Arc* arcs = (pc::Arc*)w2.take(arcs_b);
    double2* axy = (double2*)w2.take(axy_b);
    int32_t* next = (int32_t*)w2.take(link_b);
    int32_t* ring_first = (int32_t*)w2.take(link_b);
    int32_t* order = (int32_t*)w2.take(link_b);
    int32_t* info = (int32_t*)w2.take(link_b);
    unsigned long long sizes[4] = {0, 0, 0, 0};
    if (n > 0) {
        // (a record the fill pass should leave unwritten has length 0, which the stitcher refuses)
        GPK_HIP(hipMemsetAsync(arcs, 0, arcs_b, s));
        if (total_arcs > 0)
            GPK_PCLIP_BY_G(plain, nm.fill, (polygon_clip_fill_kernel<lp::LP_G_SMALL, Rule>), (polygon_clip_fill_kernel<lp::LP_G_LARGE, Rule>), a->d, b->d, arows, brows, n, (int)mode, (const int32_t*)arc_start,
                           (const int32_t*)acoord_start, arcs, axy);
        GPK_PCLIP_BY_G(plain, nm.stitch, (polygon_clip_stitch_kernel<lp::LP_G_SMALL, INNERMOST>), (polygon_clip_stitch_kernel<lp::LP_G_LARGE, INNERMOST>), n, (int)drop, (const int32_t*)arc_start, (const int32_t*)acoord_start,
                       (const pc::Arc*)arcs, (const double2*)axy, next, ring_first, order, info, valid, n_parts, n_rings, n_coords, keep, status);
        GPK_TRY(exclusive_scan_i32(n_parts, n, part_start, nullptr, tot_parts, s));
        GPK_TRY(exclusive_scan_i32(n_rings, n, ring_start, nullptr, tot_rings, s));
        GPK_TRY(exclusive_scan_i32(n_coords, n, coord_start, nullptr, tot_coords, s));
        GPK_TRY(exclusive_scan_i32(keep, n, row_at, nullptr, tot_rows, s));
        GPK_LAUNCH(nm.totals, polygon_clip_totals_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)(tot_parts + at),
                   (const unsigned long long*)(tot_rings + at), (const unsigned long long*)(tot_coords + at), (const unsigned long long*)(tot_rows + at),
                   totals_dev + 8);
        GPK_HIP(d2h_small(sizes, totals_dev + 8, sizeof sizes, s));
        GPK_HIP(sync_small(s));
    }
    if (sizes[0] > (unsigned long long)INT32_MAX || sizes[1] > (unsigned long long)INT32_MAX || sizes[2] > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: the result exceeds 2^31 - 1 parts / rings / coordinates (Arrow i32 offsets)", nm.op);
    const int64_t n_out = (int64_t)sizes[3];
    const int32_t total_parts = (int32_t)sizes[0], total_rings = (int32_t)sizes[1], total_coords = (int32_t)sizes[2];

    // ---- the result column: owned buffers, as gpk_line_clip's, plus part_off
    gpk_geoarray* r = new gpk_geoarray;
    memset(r, 0, sizeof *r);
    (void)hipGetDevice(&r->device);
    r->d.type = GPK_GEOM_MULTIPOLYGON;
    r->d.n_geoms = n_out;
    r->d.n_parts = total_parts;
    r->d.n_rings = total_rings;
    r->d.n_coords = total_coords;
    auto done = [&](int32_t rc) {
        if (rc != GPK_OK) {
            (void)hipStreamSynchronize(s);
            gpk_geoarray_free(r);
        } else {
            *out = r;
        }
        return rc;
    };
    auto alloc = [&](int slot, size_t bytes, const void** view) -> int32_t {
        void* p = nullptr;
        const hipError_t e = device_malloc(&p, bytes ? bytes : 8);
        if (e != hipSuccess) return fail(GPK_ERR_OOM, "%s: device_malloc(%zu) failed: %s", nm.op, bytes, hipGetErrorString(e));
        r->owned[slot] = p;
        *view = p;
        r->nbytes += (int64_t)bytes;
        return GPK_OK;
    };
    int32_t rc = alloc(0, sizeof(double2) * (size_t)total_coords, (const void**)&r->d.xy);
    if (rc == GPK_OK) rc = alloc(1, sizeof(int32_t) * (size_t)(n_out + 1), (const void**)&r->d.geom_off);
    if (rc == GPK_OK) rc = alloc(2, sizeof(int32_t) * (size_t)(total_parts + 1), (const void**)&r->d.part_off);
    if (rc == GPK_OK) rc = alloc(3, sizeof(int32_t) * (size_t)(total_rings + 1), (const void**)&r->d.ring_off);
    if (rc == GPK_OK && !drop && n > 0) rc = alloc(4, (size_t)((n + 7) / 8), (const void**)&r->d.validity);
    if (rc != GPK_OK) return done(rc);

    // ---- 6: offsets, emit
    if (n == 0) {
        hipError_t e = hipMemsetAsync(r->owned[1], 0, sizeof(int32_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(r->owned[2], 0, sizeof(int32_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(r->owned[3], 0, sizeof(int32_t), s);
        return done(e == hipSuccess ? GPK_OK : fail(GPK_ERR_DEVICE, "%s: %s", nm.op, hipGetErrorString(e)));
    }
    GPK_LAUNCH_OR(done, nm.offsets, polygon_clip_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int32_t*)part_start,
                  (const int32_t*)row_at, (const int32_t*)keep, (const uint8_t*)valid, n, n_out, total_parts, total_rings, total_coords,
                  (int32_t*)r->owned[1], (int32_t*)r->owned[2], (int32_t*)r->owned[3], (uint8_t*)r->owned[4], src_dev);
    if (total_rings > 0)
        GPK_PCLIP_BY_G(done, nm.emit, (polygon_clip_emit_kernel<lp::LP_G_SMALL>), (polygon_clip_emit_kernel<lp::LP_G_LARGE>), n, (const int32_t*)arc_start, (const int32_t*)acoord_start,
                       (const pc::Arc*)arcs, (const double2*)axy, (const int32_t*)next, (const int32_t*)order, (const int32_t*)part_start,
                       (const int32_t*)ring_start, (const int32_t*)coord_start, (int32_t*)r->owned[2], (int32_t*)r->owned[3], (double2*)r->owned[0]);
    if (stage_src && n_out > 0) {
        rc = copy_out(out_src, src_space, src_dev, sizeof(int32_t) * (size_t)n_out, s);
        if (rc != GPK_OK) return done(rc);
    }
    if (out_status) {
        rc = copy_out(out_status, status_space, status, (size_t)n, s);
        if (rc != GPK_OK) return done(rc);
    }
    return done(GPK_OK);
}

}  // namespace

}  // namespace gpk
