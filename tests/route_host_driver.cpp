// route_host_driver.cpp — the routing image's arithmetic on the CPU: the host-callable routines of csrc/gpk_route.h (the cell -> block and
// bit maps, route_order, the packed third word).  A stand-alone program: tests/test_route_host.py builds it plain and with
// -fsanitize=address,undefined.  It prints one line per check and exits non-zero on the first that fails.
//
//   route_host_driver
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpk_route.h"

using namespace gpk;

static void die(const char* what, long long a = 0, long long b = 0) {
    fprintf(stderr, "route_host_driver: %s (%lld, %lld)\n", what, a, b);
    exit(1);
}

int main() {
    // 1. route_order is a bijection of [0, R * R) for every raster size that gets an image, and the cells of one
    //    word are the 8 x 4 cells of one block
    for (int logR = 6; (1 << logR) <= PIP_ROUTE_RMAX; ++logR) {
        const uint32_t R = 1u << logR, n = R * R;
        std::vector<unsigned char> seen(n, 0);
        for (uint32_t c = 0; c < n; ++c) {
            const uint32_t o = route_order(c, logR);
            if (o >= n) die("route_order leaves [0, R * R)", c, o);
            if (seen[o]) die("route_order maps two cells to one place", c, o);
            seen[o] = 1;
            const uint32_t cx = c & (R - 1u), cy = c >> logR;
            if ((o >> 5) != route_block(cx, cy, logR) || (o & 31u) != route_bit(cx, cy)) die("route_order is not block << 5 | bit", c, o);
            if (route_block(cx, cy, logR) != (cy / 4u) * (R / 8u) + cx / 8u) die("blocks are not 8 x 4 cells in block-row major order", c, o);
            if (route_bit(cx, cy) != (cy % 4u) * 8u + cx % 8u) die("a cell's bit is not its place in the block", c, o);
        }
        for (uint32_t o = 0; o < n; ++o)
            if (!seen[o]) die("route_order misses a place", o, logR);
        printf("order R=%u ok\n", R);
    }
    // 2. the block and the bit from a point's sub-cell coordinates, as the join computes them, agree with the ones from its cell —
    //    every sub-cell of every raster size
    for (int logR = 6; (1 << logR) <= PIP_ROUTE_RMAX; ++logR) {
        const uint32_t S = 8u << logR;
        for (uint32_t sy = 0; sy < S; ++sy)
            for (uint32_t sx = 0; sx < S; ++sx) {
                const uint32_t cx = sx >> 3, cy = sy >> 3;
                if (route_block_sub(sx, sy, logR) != route_block(cx, cy, logR)) die("block from sub-cell coordinates", sx, sy);
                if (route_bit_sub(sx, sy) != route_bit(cx, cy)) die("bit from sub-cell coordinates", sx, sy);
                if (((route_block_sub(sx, sy, logR) << 5) | route_bit_sub(sx, sy)) != route_order((cy << logR) | cx, logR)) die("place from sub-cell coordinates", sx, sy);
            }
        const uint32_t last = S - 1u;
        if (route_block_sub(last, last, logR) != (1u << (2 * logR - 5)) - 1u || route_bit_sub(last, last) != 31u) die("the last sub-cell is not the last bit of the last word", logR);
        printf("sub R=%u ok\n", 1u << logR);
    }
    // 3. the packed word: the largest record index with the largest owner, no owner, and the first part that is never an owner
    {
        const uint32_t rec_max = (1u << 18) - 1u;
        if (ROUTE_REC_MASK != rec_max || ROUTE_OWNER_MAX != 16383u) die("field widths");
        const uint32_t w = route_pack(rec_max, 16382u);
        if (route_rec0(w) != rec_max || route_owner(w) != 16382u) die("round trip at the largest record and owner", route_rec0(w), route_owner(w));
        if (w != 0xFFFFFFFFu) die("the largest word is not all ones", w);
        const uint32_t none = route_pack(rec_max, 16383u);
        if (route_rec0(none) != rec_max || route_owner(none) != ROUTE_NO_OWNER || (none >> 18) != 0u) die("owner 16,383 must encode none", none);
        if (route_owner(route_pack(5u, ROUTE_NO_OWNER)) != ROUTE_NO_OWNER || route_rec0(route_pack(5u, ROUTE_NO_OWNER)) != 5u) die("no owner");
        for (uint32_t owner = 0; owner < 16383u; ++owner)
            for (uint32_t rec = 0; rec <= rec_max; rec += (rec < 4u || rec + 4099u > rec_max ? 1u : 4099u)) {
                const uint32_t p = route_pack(rec, owner);
                if (route_rec0(p) != rec || route_owner(p) != owner) die("round trip", rec, owner);
            }
        if (route_owner(route_pack(0u, 0u)) != 0u || route_pack(0u, 0u) == 0u) die("owner 0 is an owner");
        printf("pack ok\n");
    }
    return 0;
}
