// gpk_route.h — the LDS routing image of a small point-in-polygon raster (R <= PIP_ROUTE_RMAX): its word format and the
// arithmetic that locates a raster cell in it, host-callable.  The index build (gpk_pipindex.hip), the one-launch point join
// (gpk_pipflow.hip) and tests/route_host_driver.cpp share these definitions.
//
// One 16-byte word describes a BLOCK of 8 x 4 raster cells: block (cy >> 2, cx >> 3), blocks in block-row major order, the
// cell's bit within its word = (cy & 3) << 3 | (cx & 7).  R is a power of two >= 8, so there are R * R / 32 words and
// cell -> block << 5 | bit (route_order) is a bit shuffle of the cell number: a bijection of [0, R * R).  One-part level-2
// records are numbered in that order, so that a cell's record is rec0 + the number of record cells below its bit.
//
// A cell is in one of four states, two mask bits (b, g):
//   (0, 0) empty   no polygon can contain a point of the cell: nothing to fetch
//   (1, 0) record  the cell carries a one-part level-2 record
//   (0, 1) gather  the cell's level-1 word must be read (list cells, two-part cells, interiors the block's owner does not
//                  cover, anything else non-empty)
//   (1, 1) own     every point of the cell is strictly inside the block's OWNER part: nothing to fetch
// The owner is the part that fills the most strictly-inside cells of the block (the lowest part number on a tie); compact
// blocks meet few polygons, so a point of an interior cell usually learns its polygon from the word it reads anyway.
// The third word packs the block's first record with the owner: an image exists only for R <= 512, so a record index is below
// 2^18, and such a right side has at most 65,536 coordinates, hence fewer than 2^14 parts that matter (a part numbered
// ROUTE_OWNER_MAX or more never becomes an owner: its cells stay `gather`).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GPK_ROUTE_FN __host__ __device__ inline
#else
#define GPK_ROUTE_FN inline
#endif

namespace gpk {

constexpr int PIP_ROUTE_RMAX = 512;
struct RouteWord {
    uint32_t bmask;  // bit i: cell i of the block is `record` or `own`
    uint32_t gmask;  // bit i: cell i of the block is `gather` or `own`
    uint32_t rec0;   // route_pack: record index of the block's first `record` cell | (owner part + 1) << 18
    uint32_t pad;
};

constexpr int ROUTE_REC_BITS = 18;                                        // rec0 < PIP_ROUTE_RMAX^2 = 2^18
constexpr uint32_t ROUTE_REC_MASK = (1u << ROUTE_REC_BITS) - 1u;
constexpr uint32_t ROUTE_OWNER_MAX = (1u << (32 - ROUTE_REC_BITS)) - 1u;  // 16,383: owners are parts 0 .. 16,382
constexpr uint32_t ROUTE_NO_OWNER = 0xFFFFFFFFu;
static_assert(PIP_ROUTE_RMAX * PIP_ROUTE_RMAX == 1 << ROUTE_REC_BITS, "a record index of an imaged raster fits the field");

GPK_ROUTE_FN uint32_t route_pack(uint32_t rec0, uint32_t owner) {  // owner: a part number, or anything >= ROUTE_OWNER_MAX for none
    return (rec0 & ROUTE_REC_MASK) | (owner < ROUTE_OWNER_MAX ? (owner + 1u) << ROUTE_REC_BITS : 0u);
}
GPK_ROUTE_FN uint32_t route_rec0(uint32_t packed) { return packed & ROUTE_REC_MASK; }
GPK_ROUTE_FN uint32_t route_owner(uint32_t packed) { return (packed >> ROUTE_REC_BITS) - 1u; }  // ROUTE_NO_OWNER when the field is 0

// raster cell (cx, cy) of an R = 1 << logR raster (logR >= 3) -> its word and its bit
GPK_ROUTE_FN uint32_t route_block(uint32_t cx, uint32_t cy, int logR) { return ((cy >> 2) << (logR - 3)) + (cx >> 3); }
GPK_ROUTE_FN uint32_t route_bit(uint32_t cx, uint32_t cy) { return ((cy & 3u) << 3) | (cx & 7u); }
// the same from a point's sub-cell coordinates (8 sub-cells per cell side: cx = sx >> 3, cy = sy >> 3), as the join computes them
GPK_ROUTE_FN uint32_t route_block_sub(uint32_t sx, uint32_t sy, int logR) { return ((sy >> 5) << (logR - 3)) + (sx >> 6); }
GPK_ROUTE_FN uint32_t route_bit_sub(uint32_t sx, uint32_t sy) { return ((sy >> 3) & 3u) << 3 | ((sx >> 3) & 7u); }
// cell number c = cy << logR | cx -> its place in image order (block << 5 | bit)
GPK_ROUTE_FN uint32_t route_order(uint32_t c, int logR) {
    const uint32_t cx = c & ((1u << logR) - 1u), cy = c >> logR;
    return (route_block(cx, cy, logR) << 5) | route_bit(cx, cy);
}

}  // namespace gpk
