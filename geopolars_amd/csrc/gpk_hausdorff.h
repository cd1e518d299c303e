// gpk_hausdorff.h — the per-row rules of gpk_hausdorff_distance (include/geopolars_hip.h states the contract, DESIGN.md section 4.3m the
// schedules): the discrete Hausdorff distance between the boundaries of two rows, H = max(h(A -> B), h(B -> A)).
//
//   samples    a row is its coordinate sequences (RowSeqs, gpk_pairdist.h; a POINT is one sequence of one coordinate).  With
//              subdivisions = k every coordinate c owns k slots j = 0 .. k - 1: slot 0 is the vertex, slot j > 0 the double
//              p.x + (double)j * ((q.x - p.x) / (double)k) (q = coordinate c + 1; the same for y), every operation rounded on its own.
//              The slots j > 0 of a coordinate that ends its sequence do not exist; rows without sequence table (POINT, MULTIPOINT)
//              have slot 0 only.  Samples = existing slots: (n - q) * k + q for n coordinates in q non-empty sequences.
//   h(L -> W)  the largest, over the samples of L, of the smallest point-segment term over the segments of W (undensified; one
//              segment per coordinate: (c, c + 1) inside its sequence, else the degenerate (c, c)).  Terms are pair_seg_dist2
//              fractions, compared by cross-multiplication (frac_less): a later term replaces the running minimum only when strictly
//              smaller, a later minimum the running maximum only when strictly larger.
//   H          pick_max(h(A -> B), h(B -> A)): the larger fraction; of two fractions of equal value the one with the larger numerator
//              — a rule that does not look at the order of its arguments, so H(a, b) and H(b, a) have the same bits.  One division
//              and one square root.  No substitution for a computed zero: identical rows give exactly 0.0.
//   cost       s_A * n_B + s_B * n_A (samples times walked segments, both directions) in 64 bits; rows above HD_LARGE_COST are
//              finished by the work-group kernel.  HD_LARGE_COST starts at PD_LARGE_COST: a first value, NOT swept.
//
// The rules below are plain C++, and so are the routines they stand on (Frac, frac_less, pair_seg_dist2: gpk_frac.h): the kernels
// (gpk_hausdorff.hip) and a host program (tests/hausdorff_host_driver.cpp) compile the same functions.  The schedules — which lane takes
// which sample, the butterfly, the work-group fold — are device code; the host program restates them with arrays.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/geopolars_hip.h"
#include "gpk_frac.h"

#if defined(__HIPCC__)
#define GPK_HD_FN __host__ __device__ __forceinline__
#else
#define GPK_HD_FN inline
#endif

namespace gpk {
namespace hd {

constexpr int MAX_SUBDIVISIONS = GPK_MAX_SUBDIVISIONS;
constexpr int64_t HD_LARGE_COST = PD_LARGE_COST;  // a first value, not swept

// slot j (0 <= j < k) between the ordinates p and q of two consecutive coordinates
GPK_HD_FN double sample_coord(double p, double q, int j, int k) { return p + (double)j * ((q - p) / (double)k); }

// samples of n coordinates in q non-empty sequences (sequenced: the row has a sequence table)
GPK_HD_FN int64_t sample_count(int64_t n, int64_t q, int k, bool sequenced) { return sequenced ? (n - q) * (int64_t)k + q : n; }
// s_A * n_B + s_B * n_A of a pair with coordinates on both sides; any value above HD_LARGE_COST stands for "large" (a factor above the
// threshold decides alone, so the products stay far inside 64 bits)
GPK_HD_FN int64_t cost(int64_t sa, int64_t na, int64_t sb, int64_t nb) {
    const int64_t cap = HD_LARGE_COST + 1;
    if (sa > cap || na > cap || sb > cap || nb > cap) return cap;
    return sa * nb + sb * na;
}

GPK_HD_FN Frac no_min() { return Frac{INFINITY, 1.0}; }  // above every term
GPK_HD_FN Frac no_max() { return Frac{-1.0, 1.0}; }      // below every term (terms are >= 0)
GPK_HD_FN void see_min(Frac& m, const Frac& t) {
    if (frac_less(t, m)) m = t;
}
GPK_HD_FN void see_max(Frac& m, const Frac& t) {
    if (frac_less(m, t)) m = t;
}
GPK_HD_FN Frac pick_max(const Frac& a, const Frac& b) {
    const bool a_first = a.num > b.num || (a.num == b.num && a.den >= b.den);  // among fractions of equal value
    const bool take_b = frac_less(a, b) || (!frac_less(b, a) && !a_first);
    return Frac{take_b ? b.num : a.num, take_b ? b.den : a.den};  // (selects on the fields: no address of a or b is taken)
}
GPK_HD_FN double result(const Frac& h) { return sqrt(h.num / h.den); }

}  // namespace hd
}  // namespace gpk
