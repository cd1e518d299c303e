// gpk_clipcall.h — what the pair calls that return a new column share around their own kernels (gpk_line_clip in gpk_lineclip.hip;
// gpk_polygon_clip and gpk_polygon_union through gpk_polyclip_run.h): the argument checks, the staging of host row lists and of
// out_src, the grid of one group per pair, the read-back of scan totals and the kernel that writes geom_offsets, the validity bitmap
// and the compaction map.  Profile stage names come from the caller.  The result column itself: gpk_column.h.
#pragma once

#include <climits>

#include "gpk_column.h"
#include "gpk_common.h"

namespace gpk {

namespace {

// how one side of the pairs is called in messages: its row list and its rows ({"line_rows", "line rows"}, {"a_rows", "rows of a"})
struct ClipSide {
    const char *rows, *what;
};

// The checks of a pair call, the plain arguments first: a bad mode or flag is refused whatever else is handed over.  families(ta, tb):
// the caller's check of the two geometry types, at its place in the order.
template <class Families>
int32_t clip_prologue(const char* op, const ClipSide& sa, const ClipSide& sb, bool mode_ok, int32_t mode, int32_t flags, const int32_t* out_src,
                      int64_t n_rows, const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, gpk_geoarray** out,
                      Families families) {
    if (!mode_ok) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: unknown mode %d", op, mode);
    if (flags & ~GPK_CLIP_DROP_EMPTY) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", op, flags);
    if (out_src && !(flags & GPK_CLIP_DROP_EMPTY))
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: out_src is the map of GPK_CLIP_DROP_EMPTY, which is not set", op);
    if (n_rows < 0 || n_rows > (int64_t)INT32_MAX) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: %lld pairs", op, (long long)n_rows);
    if (!a || !b || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    GPK_TRY(families(a->d.type, b->d.type));
    if (!a_rows && n_rows != a->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: %lld pairs without %s but %lld %s", op, (long long)n_rows, sa.rows, (long long)a->d.n_geoms, sa.what);
    if (!b_rows && n_rows != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: %lld pairs without %s but %lld %s", op, (long long)n_rows, sb.rows, (long long)b->d.n_geoms, sb.what);
    return require_device();
}

// Host row lists and a host out_src are staged in the call's Scratch; device ones are used where they are.
struct ClipLists {
    const uint32_t *a_rows, *b_rows;
    int32_t* src;     // where the kernels write the compaction map (nullptr: none asked for)
    bool src_staged;  // ... which the caller copies out to out_src at the end
};
// records the carves (src: `words` entries; without pairs a row list is never read and stays the caller's); the caller uploads the host
// lists with sc.upload after commit()
inline void clip_lists_plan(Scratch& sc, const uint32_t* a_rows, const uint32_t* b_rows, int32_t rows_space, int32_t* out_src, int32_t src_space, int64_t n,
                            size_t words, ClipLists* out) {
    sc.stage_in(out->a_rows, a_rows, n > 0 ? rows_space : GPK_MEM_DEVICE, (size_t)n);
    sc.stage_in(out->b_rows, b_rows, n > 0 ? rows_space : GPK_MEM_DEVICE, (size_t)n);
    sc.stage(out->src, out_src, src_space, words);
    out->src_staged = out_src && src_space != GPK_MEM_DEVICE;
}

// the row of pair k on one side: rows[k] or k; an entry past the column's end: -1 (a null row)
__device__ __forceinline__ int64_t row_of(const uint32_t* __restrict__ rows, int64_t k, int64_t n_geoms) {
    const int64_t r = rows ? (int64_t)rows[k] : k;
    return r < n_geoms ? r : -1;
}

// one group of G lanes per pair, uncapped
inline dim3 pair_grid(int64_t n, int G) { return dim3((unsigned)((n + (256 / G) - 1) / (256 / G))); }

// the kernel at the pairs' group size (G, n and s of the calling scope): small and large are its instantiations for lp::LP_G_SMALL and
// lp::LP_G_LARGE, each in parentheses
#define GPK_LAUNCH_BY_G(name, small, large, ...)                                   \
    do {                                                                           \
        if (G == lp::LP_G_SMALL)                                                   \
            GPK_LAUNCH(name, small, pair_grid(n, G), dim3(256), 0, s, __VA_ARGS__); \
        else                                                                       \
            GPK_LAUNCH(name, large, pair_grid(n, G), dim3(256), 0, s, __VA_ARGS__); \
    } while (0)

// up to four 64-bit scan totals in one record; a pointer that is not given reads as 0
__global__ void clip_totals_kernel(const unsigned long long* __restrict__ t0, const unsigned long long* __restrict__ t1,
                                   const unsigned long long* __restrict__ t2, const unsigned long long* __restrict__ t3,
                                   unsigned long long* __restrict__ out) {
    if (threadIdx.x == 0) {
        out[0] = t0 ? *t0 : 0;
        out[1] = t1 ? *t1 : 0;
        out[2] = t2 ? *t2 : 0;
        out[3] = t3 ? *t3 : 0;
    }
}
// ... gathered at record_dev (32 bytes of scratch) and read back: one launch, one copy, one wait of the stream
inline int32_t clip_read_totals(const char* name, const unsigned long long* t0, const unsigned long long* t1, const unsigned long long* t2,
                                const unsigned long long* t3, unsigned long long* record_dev, unsigned long long out[4], hipStream_t s) {
    GPK_LAUNCH(name, clip_totals_kernel, dim3(1), dim3(64), 0, s, t0, t1, t2, t3, record_dev);
    GPK_HIP(d2h_small(out, record_dev, 4 * sizeof(unsigned long long), s));
    GPK_HIP(sync_small(s));
    return GPK_OK;
}

// geom_offsets, validity and the compaction map.  row_at[k]: the output row of pair k when it stays (keep[k]).  The first lane closes
// every offsets level there is: geom -> part -> ring -> coordinate with part_off, geom -> ring -> coordinate without it (a
// MULTILINESTRING result, whose total_parts is unused).
__global__ __launch_bounds__(256) void clip_offsets_kernel(const int32_t* __restrict__ part_start, const int32_t* __restrict__ row_at,
                                                           const int32_t* __restrict__ keep, const uint8_t* __restrict__ valid, int64_t n, int64_t n_out,
                                                           int32_t total_parts, int32_t total_rings, int32_t total_coords,
                                                           int32_t* __restrict__ geom_off, int32_t* __restrict__ part_off, int32_t* __restrict__ ring_off,
                                                           uint8_t* __restrict__ validity, int32_t* __restrict__ out_src) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) {
        if (part_off) {
            geom_off[n_out] = total_parts;
            part_off[total_parts] = total_rings;
        } else {
            geom_off[n_out] = total_rings;
        }
        ring_off[total_rings] = total_coords;
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
inline int32_t clip_write_offsets(const char* name, const int32_t* part_start, const int32_t* row_at, const int32_t* keep, const uint8_t* valid, int64_t n,
                                  int64_t n_out, int32_t total_parts, int32_t total_rings, int32_t total_coords, Column& col, int32_t* src, hipStream_t s) {
    GPK_LAUNCH(name, clip_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part_start, row_at, keep, valid, n, n_out, total_parts,
               total_rings, total_coords, col.geom_off(), col.part_off(), col.ring_off(), col.validity(), src);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk
