// gpk_geotake.h — gather of geometry rows (gpk_geoarray_take / gpk_geoarray_filter): the rule, host-callable.  Kernels and the
// driver: gpk_geotake.hip.  Contract: include/geopolars_hip.h.
//
// A geometry column is up to three offsets levels over a coordinate buffer (geom -> [part ->] [ring ->] coordinate), and the children
// of a row are contiguous at EVERY level.  So a row slot i that reads source row j owns, at level l, the source range
// [src_lo[l][i], src_lo[l][i] + cnt[l][i]) — row_ranges() below, one walk down the first and last offset of each level — and, after an
// exclusive scan of cnt[l] over the slots, the output range that starts at dst_lo[l][i].  A slot that yields nothing (an index
// outside [0, n), a row the mask drops) has cnt == 0 at every level: an empty row.
//
// The fill works in OUTPUT order.  One strip is STRIP consecutive output elements of one level (coordinates, or the entries of an
// offsets level).  The row of every strip's first element comes from one bisection of dst_lo a strip (the level's strip table); the
// row starts from there to the next strip's first row are the strip's WINDOW (staged in LDS on the device when at most WINDOW of
// them; bisected where they are otherwise — thousands of empty rows may end inside one strip).  An element's row is the LAST row that
// starts at or before it: of a run of rows with one start all but the last are empty, so the search skips them.  Then
//     coordinate:      out[e] = src[src_lo[r] + (e - dst_lo[r])]
//     offsets entry:   out[e] = src_off[src_lo[r] + (e - dst_lo[r])] - src_child_lo[r] + dst_child_lo[r]
// the same locate step with another payload (Payload::value).  The window holds, beside every row's start, its src_lo[r] - dst_lo[r]:
// what separates the located row from the load of its element is then LDS only.  The entry that closes an offsets level
// (out[total] = the child total) is written with the level-0 offsets, by the row pass.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GPK_GT_FN __host__ __device__ inline
#else
#define GPK_GT_FN inline
#endif

namespace gpk {
namespace gt {

constexpr int LANES = 256;    // lanes of a work-group
constexpr int PER_LANE = 4;   // elements a lane moves
constexpr int STRIP = LANES * PER_LANE;  // 1024 output elements a work-group
constexpr int WINDOW = 2048;  // row starts a strip stages (16 KB of LDS with the shifts); a strip with more rows bisects in global memory
constexpr int MAX_LEVELS = 3;

// 16 bytes moved as they are: a coordinate with its NaN payloads and signed zeros
struct alignas(16) Bits16 {
    uint64_t lo, hi;
};

// the source ranges of row j at every level: lo[l], hi[l] index the children of level l (level `levels - 1`: coordinates)
GPK_GT_FN void row_ranges(const int32_t* const off[MAX_LEVELS], int levels, int64_t j, int32_t lo[MAX_LEVELS], int32_t hi[MAX_LEVELS]) {
    int64_t a = j, b = j + 1;
    for (int l = 0; l < levels; ++l) {
        lo[l] = off[l][a];
        hi[l] = off[l][b];
        a = lo[l];
        b = hi[l];
    }
}

// the row starts a strip looks at: rows first .. last of `start` (dst_lo of the level above), through `win` (a copy of
// start[first .. last]) when there is one
struct Rows {
    const int32_t* start;
    const int32_t* win;
    const int32_t* shift_win;  // with win: src_lo[r] - start[r] of the same rows (what an element adds to its number to find its source)
    int64_t first, last;
    GPK_GT_FN int32_t at(int64_t r) const { return win ? win[r - first] : start[r]; }
    GPK_GT_FN int64_t shift(int64_t r, const int32_t* src_lo) const {
        return win ? (int64_t)shift_win[r - first] : (int64_t)src_lo[r] - (int64_t)start[r];
    }
    // the last row of [first, last] that starts at or before e (at(first) <= e)
    GPK_GT_FN int64_t find(int64_t e) const {
        int64_t lo = first, hi = last;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if ((int64_t)at(mid) <= e)
                lo = mid;
            else
                hi = mid - 1;
        }
        return lo;
    }
    // ... for the element after one of row r: the same row unless the next one has begun
    GPK_GT_FN int64_t next(int64_t r, int64_t e) const { return (r >= last || (int64_t)at(r + 1) > e) ? r : find(e); }
};

// The strip table of a level whose n_rows rows start at start[0 .. n_rows) (start[0] == 0): entry s is the row of the strip's first
// element, s * STRIP — one bisection a strip, made once (a lane per strip on the device) instead of by every work-group of the fill.
GPK_GT_FN int32_t strip_first_row(const int32_t* start, int64_t n_rows, int64_t strip) {
    const Rows all{start, nullptr, nullptr, 0, n_rows - 1};
    return (int32_t)all.find(strip * STRIP);
}
// The rows of strip s of n_strips: from its first element's row to the next strip's (the row of the strip's last element or a later
// one: the runs of empty rows in between only widen the window); the last strip looks up to the last row.
GPK_GT_FN Rows strip_rows(const int32_t* start, int64_t n_rows, const int32_t* first_row, int64_t s, int64_t n_strips) {
    return Rows{start, nullptr, nullptr, first_row[s], s + 1 < n_strips ? (int64_t)first_row[s + 1] : n_rows - 1};
}
// a source offset moved to the output: the row's children begin at src_child_lo there and at dst_child_lo here
GPK_GT_FN int32_t rebase(int32_t src_off, int32_t src_child_lo, int32_t dst_child_lo) {
    return (int32_t)((int64_t)src_off - (int64_t)src_child_lo + (int64_t)dst_child_lo);
}

// ---- the two payloads of the locate step ----------------------------------------------------------------------------------------
// Coordinates: 16-byte elements.  Lane t takes elements t, t + LANES, ...: every load / store instruction of a wave covers 1 KiB of
// consecutive output, and of consecutive source within a row's run.
struct CoordPayload {
    typedef Bits16 T;
    static constexpr bool CONSECUTIVE = false;
    const Bits16* src;
    Bits16* dst;
    const int32_t* src_lo;  // [row]: the row's first coordinate in the source
    GPK_GT_FN Bits16 value(int64_t r, int64_t src_e) const { return src[src_e]; }
};
// An offsets level: 4-byte elements, four consecutive ones per lane — one 16-byte store.
struct OffsetPayload {
    typedef int32_t T;
    static constexpr bool CONSECUTIVE = true;
    const int32_t* src;  // the source's offsets of this level
    int32_t* dst;
    const int32_t* src_lo;        // [row]: the row's first entry of this level in the source
    const int32_t* src_child_lo;  // [row]: its first child there
    const int32_t* dst_child_lo;  // [row]: its first child in the output
    GPK_GT_FN int32_t value(int64_t r, int64_t src_e) const { return rebase(src[src_e], src_child_lo[r], dst_child_lo[r]); }
};

// element k of lane t of the strip that begins at e0
template <class Payload>
GPK_GT_FN int64_t lane_element(int64_t e0, int t, int k) {
    return Payload::CONSECUTIVE ? e0 + (int64_t)t * PER_LANE + k : e0 + (int64_t)k * LANES + t;
}

// What lane t of a strip computes: its PER_LANE elements of [e0, e_end), v[k] valid where the return value has bit k.
template <class Payload>
GPK_GT_FN unsigned lane_values(const Payload& p, const Rows& rows, int64_t e0, int64_t e_end, int t, typename Payload::T v[PER_LANE]) {
    unsigned have = 0;
    int64_t r = -1;
    for (int k = 0; k < PER_LANE; ++k) {
        const int64_t e = lane_element<Payload>(e0, t, k);
        if (e >= e_end) continue;
        r = (Payload::CONSECUTIVE && r >= 0) ? rows.next(r, e) : rows.find(e);
        v[k] = p.value(r, e + rows.shift(r, p.src_lo));  // the source address: src_lo[r] + (e - dst_lo[r])
        have |= 1u << k;
    }
    return have;
}

}  // namespace gt
}  // namespace gpk
