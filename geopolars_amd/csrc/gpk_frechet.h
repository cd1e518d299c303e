// gpk_frechet.h — the per-cell rules of gpk_frechet_distance (include/geopolars_hip.h states the contract, DESIGN.md section 4.3m the
// schedules): the discrete Frechet distance of two LINESTRING rows over their sample sequences P (n' samples) and Q (m' samples),
//     c(0, 0) = d(0, 0),   c(i, j) = max(d(i, j), min(c(i - 1, j), c(i, j - 1), c(i - 1, j - 1)))   (missing neighbours left out),
//     result  = sqrt(c(n' - 1, m' - 1)),
// on squared distances d = dx * dx + dy * dy in f64.
//
//   samples    n coordinates give (n - 1) * k + 1 samples: sample t is slot j = t % k of coordinate t / k, slot 0 the vertex, slot j > 0
//              the double p.x + (double)j * ((q.x - p.x) / (double)k) (q the next coordinate; the same for y), every operation rounded
//              on its own.  Counts are 64-bit.
//   cells      max and min only select among the d values, so the table is the same whichever side is walked and in whichever order
//              independent cells are filled: frechet(a, b) and frechet(b, a) are the same double, and 0 exactly iff every d on some
//              monotone path is an exact 0.  A missing neighbour is +infinity; the cell above-left of (0, 0) is 0, which makes
//              c(0, 0) = d(0, 0) without a special case.
//
// Schedule (gpk_frechet.hip): a skewed wavefront.  The shorter side is walked (R samples, the rows of the table), the longer one lies
// across the lanes (C samples, the columns) in strips of G columns.  In a strip lane l owns column j0 + l and computes cell (t - l, j0 + l)
// at step t: the value to its left is lane l - 1's previous cell (one __shfl_up), the diagonal the value it received a step earlier,
// the value above its own previous cell.  The walked side's samples enter at lane 0 and travel down the same shift register (two more
// __shfl_up), so a strip needs no barrier and no copy of the walked side.  The last lane's column goes to a boundary column of R doubles
// in LDS and is lane 0's left input in the next strip (in place: entry i is read by lane 0 at step i and overwritten by lane G - 1 at step i + G - 1, G - 1 steps later).
//   frechet_kernel<G>        G = 8 or 32 lanes per row (pairdist_group_size), one group per row, a boundary column of FR_GROUP_SHORT
//                            doubles per group.  Rows above FR_LARGE_COST cells are appended to a list.  FR_LARGE_COST = 2^14 is a
//                            first value, NOT swept; it was chosen so that the shorter side of a row that stays here has at most
//                            sqrt(2^14) = FR_GROUP_SHORT samples, which keeps the block's boundary columns at 32 KB for G = 8.
//   frechet_large_kernel     the listed rows: ONE WAVE per row, 64 columns a strip, and the whole work-group's LDS behind it: a
//                            boundary column of GPK_FRECHET_MAX_SHORT = 16384 doubles (128 KB of the 160 KB).  The work-group is that
//                            one wave.  The choice against the alternatives (four rows a work-group: a quarter of the cap each;
//                            strips pipelined wave to wave through LDS: flags and spinning between waves): nothing waits on another
//                            wave, so there is nothing to deadlock.  Its cost: one resident wave per compute unit, so a listed row runs
//                            at the latency of one dependent chain (three shuffles and about ten f64 operations a step) and the unit's
//                            other SIMDs idle; a column of long rows is bound by R * C / 64 such steps per row over 256 rows at a time.
// Rows whose shorter side has more than GPK_FRECHET_MAX_SHORT samples are not computed (NaN, counted in n_over).
//
// The rules below are plain C++: the kernels and a host program (tests/hausdorff_host_driver.cpp) compile the same functions.  The
// wavefront itself (frechet_table, gpk_frechet.hip) is device code; the host program restates it with the lanes' registers as arrays.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/geopolars_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GPK_FR_FN __host__ __device__ __forceinline__
#else
#define GPK_FR_FN inline
#endif

namespace gpk {
namespace fr {

constexpr int MAX_SUBDIVISIONS = GPK_MAX_SUBDIVISIONS;
constexpr int64_t FR_LARGE_COST = 1 << 14;  // cells; a first value, not swept
constexpr int FR_GROUP_SHORT = 128;         // boundary column of a lane group: FR_GROUP_SHORT^2 == FR_LARGE_COST
constexpr int64_t MAX_SHORT = GPK_FRECHET_MAX_SHORT;
static_assert((int64_t)FR_GROUP_SHORT * FR_GROUP_SHORT >= FR_LARGE_COST, "a row below FR_LARGE_COST must fit the group's boundary column");

GPK_FR_FN int64_t sample_count(int64_t n_coords, int k) { return n_coords > 0 ? (n_coords - 1) * (int64_t)k + 1 : 0; }
// slot j (0 < j < k) after ordinate p, `step` = (q - p) / (double)k of the segment (p, q)
GPK_FR_FN double seg_step(double p, double q, int k) { return (q - p) / (double)k; }
GPK_FR_FN double sample_coord(double p, double step, int j) { return p + (double)j * step; }
GPK_FR_FN double dist2(double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy;
}
GPK_FR_FN double cell(double d, double up, double left, double diag) { return fmax(d, fmin(fmin(up, left), diag)); }
GPK_FR_FN double result(double c) { return sqrt(c); }

}  // namespace fr
}  // namespace gpk
