// gpk_frac.h — squared point-segment distances kept as fractions, in plain C++ for the device and the host alike: the kernels of
// gpk_distance.h / gpk_pairdist.h / gpk_hausdorff.hip and the host program tests/hausdorff_host_driver.cpp compile these very functions.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GPK_FRAC_FN __host__ __device__ __forceinline__
#else
#define GPK_FRAC_FN inline
#endif

namespace gpk {

// rows whose n_A * n_B exceeds this go to the work-group schedule.  A first value, not swept: DESIGN.md 4.3c lists what was measured
constexpr int64_t PD_LARGE_COST = 1 << 16;

// a squared distance num / den: the per-segment work has no division; fractions are compared by cross-multiplication (gpk_distance.h)
struct Frac {
    double num, den;
};
GPK_FRAC_FN bool frac_less(const Frac& a, const Frac& b) { return a.num * b.den < b.num * a.den; }

// Squared distance from p to segment (s, e) as a fraction, as segment_dist2 (gpk_distance.h) but with the cross product
// evaluated by Kahan's fma algorithm: within 1.5 ulp of the exact product difference, and zero only when that is zero.
GPK_FRAC_FN Frac pair_seg_dist2(double px, double py, double sx, double sy, double ex, double ey) {
    const double dx = ex - sx, dy = ey - sy, qx = px - sx, qy = py - sy;
    const double d2 = dx * dx + dy * dy;
    const double dot = qx * dx + qy * dy;
    if (d2 == 0.0 || dot <= 0.0) return Frac{qx * qx + qy * qy, 1.0};
    if (dot >= d2) {
        const double rx = px - ex, ry = py - ey;
        return Frac{rx * rx + ry * ry, 1.0};
    }
    const double w = qy * dx;
    const double cross = __builtin_fma(qx, dy, -w) + __builtin_fma(-qy, dx, w);
    return Frac{cross * cross, d2};
}

}  // namespace gpk
