// gpk_geodesic.h — the geodesic problems on WGS84, host and device: what geo's GeodesicLength, GeodesicArea,
// GeodesicDistance, GeodesicBearing and GeodesicDestination compute through geographiclib-rs, and the metres between two points by
// the two other methods of gpk_geodesic_length.
//   inverse   (lon1, lat1, lon2, lat2) -> s12 [m], azi1, azi2 [degrees, forward, clockwise from north, in [-180, 180]], the reduced
//             length m12 [m] and S12 [m^2], the area between the edge and the equator (positive when the edge runs east on the
//             northern side: the S12 of a counter-clockwise ring sum to MINUS its area)
//   direct    (lon1, lat1, azi1, s12) -> (lon2, lat2, azi2), lon2 in [-180, 180]
//   transit   the +-1 / 0 prime-meridian crossing count of an edge, for the area reduction of a ring
//   haversine_m, vincenty_m   (lon1, lat1, lon2, lat2) -> metres, geo's HaversineLength / VincentyLength per segment
// Restated from the published algorithm (C. F. F. Karney, "Algorithms for geodesics", J. Geodesy 87, 2013, and GeographicLib's
// order-6 series): reduced latitudes, a starting azimuth (spherical, or the astroid solution near the antipode), Newton's method
// on lambda12(alp1) with bisection as the fallback, then the distance integral by Clenshaw summation, carried on to the azimuths and
// to the area integral I4 (the C4 series by Clenshaw summation; for edges that are not long the c^2 (alp2 - alp1) part comes from
// the spherical-excess formula, which does not cancel).  The direct problem reverts the distance integral with the C1p series.
// This is the library's one inverse: gpk_geodesic_length(GPK_GEODESIC_KARNEY) sums inverse<false>(...).s12 over the segments
// (gpk_lineal_ops.hip), so gpk_geodesic_inverse and the perimeter give its bits.
// Plain C++: no HIP type appears here, so a host program can include the file and run the very code the kernels run
// (tests/geodesic_host_driver.cpp).  Under hipcc every function is __host__ __device__.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GPK_GEO_FN __host__ __device__ inline
#else
#define GPK_GEO_FN inline
#endif

namespace gpk {
namespace geodesic {

#define KQ GPK_GEO_FN
#define K_A 6378137.0
#define K_F (1.0 / 298.257223563)
#define K_F1 (1.0 - K_F)
#define K_E2 (K_F * (2.0 - K_F))
#define K_EP2 (K_E2 / (K_F1 * K_F1))
#define K_N (K_F / (2.0 - K_F))
#define K_B (K_A * K_F1)
#define K_PI 3.14159265358979323846
#define K_DEGREE (K_PI / 180.0)
#define K_TINY 1.4916681462400413e-154 /* sqrt(DBL_MIN) */
#define K_TOL0 2.220446049250313e-16   /* DBL_EPSILON */
#define K_TOL1 (200.0 * K_TOL0)
#define K_TOL2 1.4901161193847656e-08  /* sqrt(DBL_EPSILON) */
#define K_TOLB (K_TOL0 * K_TOL2)
#define K_XTHRESH (1000.0 * K_TOL2)
#define K_ETOL2 (0.1 * K_TOL2 / sqrt(fmax(0.001, fabs(K_F)) * fmin(1.0, 1.0 - K_F / 2.0) / 2.0))
#define K_MAXIT1 20
#define K_MAXIT2 83
#define K_C2 40589732499314.76     /* authalic radius squared, (a^2 + b^2 atanh(e) / e) / 2 = 40589732499314.75999814 */

constexpr double AREA0 = 510065621724088.5;          /* the ellipsoid's area, 4 pi c^2 = 510065621724088.5093 */

using std::signbit;

struct Inverse {
    double s12, azi1, azi2, m12, S12;
};
struct Direct {
    double lon2, lat2, azi2;
};

/* ---- Karney's inverse geodesic on WGS84 (C. F. F. Karney, "Algorithms for geodesics", J. Geodesy 87, 2013; the order-6
 * series and the Newton / bisection scheme of GeographicLib's Geodesic::Inverse, which geo 0.27 reaches through the
 * geographiclib-rs crate) ------------------------------------------------------------------------------------------------------- */
KQ double k_sq(double x) { return x * x; }
KQ void k_norm2(double* s, double* c) {
    const double r = hypot(*s, *c);
    *s /= r;
    *c /= r;
}
KQ double k_sumx(double u, double v, double* t) {
    const double s = u + v;
    double up = s - v, vpp = s - up;
    up -= u;
    vpp -= v;
    *t = s != 0.0 ? 0.0 - (up + vpp) : s;
    return s;
}
KQ double k_ang_round(double x) {
    const double z = 1.0 / 16.0;
    double y = fabs(x);
    y = y < z ? z - (z - y) : y;
    return copysign(y, x);
}
KQ double k_ang_diff(double x, double y, double* e) {
    double t;
    double d = k_sumx(remainder(-x, 360.0), remainder(y, 360.0), &t);
    d = k_sumx(remainder(d, 360.0), t, &t);
    if (d == 0.0 || fabs(d) == 180.0) d = copysign(d, t == 0.0 ? y - x : -t);
    *e = t;
    return d;
}
KQ void k_sincosd(double x, double* sinx, double* cosx) {
    int q = 0;
    double r = remquo(x, 90.0, &q);
    r *= K_DEGREE;
    const double s = sin(r), c = cos(r);
    double sx, cx;
    switch ((unsigned)q & 3u) {
        case 0u: sx = s; cx = c; break;
        case 1u: sx = c; cx = -s; break;
        case 2u: sx = -s; cx = -c; break;
        default: sx = -c; cx = s; break;
    }
    cx += 0.0;
    if (sx == 0.0) sx = copysign(sx, x);
    *sinx = sx;
    *cosx = cx;
}
/* sum of c[k] sin(2 k x), k = 1 .. n (Clenshaw) */
KQ double k_sin_series(double sinx, double cosx, const double* c, int n) {
    const double ar = 2.0 * (cosx - sinx) * (cosx + sinx);
    c += n + 1;
    double y0 = (n & 1) ? *--c : 0.0, y1 = 0.0;
    n /= 2;
    while (n--) {
        y1 = ar * y0 - y1 + *--c;
        y0 = ar * y1 - y0 + *--c;
    }
    return 2.0 * sinx * cosx * y0;
}
KQ double k_A1m1f(double eps) {
    const double e2 = eps * eps, t = e2 * (e2 * (e2 + 4.0) + 64.0) / 256.0;
    return (t + eps) / (1.0 - eps);
}
KQ void k_C1f(double eps, double* c) {
    const double e2 = eps * eps;
    double d = eps;
    c[1] = d * ((6.0 - e2) * e2 - 16.0) / 32.0;
    d *= eps;
    c[2] = d * ((64.0 - 9.0 * e2) * e2 - 128.0) / 2048.0;
    d *= eps;
    c[3] = d * (9.0 * e2 - 16.0) / 768.0;
    d *= eps;
    c[4] = d * (3.0 * e2 - 5.0) / 512.0;
    d *= eps;
    c[5] = -7.0 * d / 1280.0;
    d *= eps;
    c[6] = -7.0 * d / 2048.0;
}
KQ double k_A2m1f(double eps) {
    const double e2 = eps * eps, t = e2 * (e2 * (-11.0 * e2 - 28.0) - 192.0) / 256.0;
    return (t - eps) / (1.0 + eps);
}
KQ void k_C2f(double eps, double* c) {
    const double e2 = eps * eps;
    double d = eps;
    c[1] = d * (e2 * (e2 + 2.0) + 16.0) / 32.0;
    d *= eps;
    c[2] = d * (e2 * (35.0 * e2 + 64.0) + 384.0) / 2048.0;
    d *= eps;
    c[3] = d * (15.0 * e2 + 80.0) / 768.0;
    d *= eps;
    c[4] = d * (7.0 * e2 + 35.0) / 512.0;
    d *= eps;
    c[5] = 63.0 * d / 1280.0;
    d *= eps;
    c[6] = 77.0 * d / 2048.0;
}
KQ double k_A3f(double eps) {
    const double n = K_N;
    double y = -3.0 / 128.0;
    y = y * eps + (-2.0 * n - 3.0) / 64.0;
    y = y * eps + ((-n - 3.0) * n - 1.0) / 16.0;
    y = y * eps + ((3.0 * n - 1.0) * n - 2.0) / 8.0;
    y = y * eps + (n - 1.0) / 2.0;
    y = y * eps + 1.0;
    return y;
}
KQ void k_C3f(double eps, double* c) {
    const double n = K_N;
    double m = eps;  /* eps^l */
    c[1] = m * ((((3.0 / 128.0) * eps + (2.0 * n + 5.0) / 128.0) * eps + ((-n + 3.0) * n + 3.0) / 64.0) * eps + ((-n) * n + 1.0) / 8.0) * eps
           + m * ((-n + 1.0) / 4.0);
    m *= eps;
    c[2] = m * ((((5.0 / 256.0) * eps + (n + 3.0) / 128.0) * eps + ((-3.0 * n - 2.0) * n + 3.0) / 64.0) * eps + ((n - 3.0) * n + 2.0) / 32.0);
    m *= eps;
    c[3] = m * (((7.0 / 512.0) * eps + (-10.0 * n + 9.0) / 384.0) * eps + ((5.0 * n - 9.0) * n + 5.0) / 192.0);
    m *= eps;
    c[4] = m * ((7.0 / 512.0) * eps + (-14.0 * n + 7.0) / 512.0);
    m *= eps;
    c[5] = m * (21.0 / 2560.0);
}
/* s12b (distance / b) and m12b (reduced length / b) of the arc sig1 .. sig2; *m0 = A1 - A2 */
KQ void k_lengths(double eps, double sig12, double ssig1, double csig1, double dn1, double ssig2, double csig2, double dn2, double* s12b, double* m12b,
               double* m0) {
    double ca[7], cb[7];
    k_C1f(eps, ca);
    k_C2f(eps, cb);
    const double A1 = k_A1m1f(eps), A2 = k_A2m1f(eps);
    const double B1 = k_sin_series(ssig2, csig2, ca, 6) - k_sin_series(ssig1, csig1, ca, 6);
    const double B2 = k_sin_series(ssig2, csig2, cb, 6) - k_sin_series(ssig1, csig1, cb, 6);
    *s12b = (1.0 + A1) * (sig12 + B1);
    *m0 = A1 - A2;
    const double J12 = (A1 - A2) * sig12 + ((1.0 + A1) * B1 - (1.0 + A2) * B2);
    *m12b = dn2 * (csig1 * ssig2) - dn1 * (ssig1 * csig2) - csig1 * csig2 * J12;
}
KQ double k_astroid(double x, double y) {
    const double p = x * x, q = y * y, r = (p + q - 1.0) / 6.0;
    if (q == 0.0 && r <= 0.0) return 0.0;
    const double S = p * q / 4.0, r2 = r * r, r3 = r * r2, disc = S * (S + 2.0 * r3);
    double u = r;
    if (disc >= 0.0) {
        double T3 = S + r3;
        T3 += T3 < 0.0 ? -sqrt(disc) : sqrt(disc);
        const double T = cbrt(T3);
        u += T + (T != 0.0 ? r2 / T : 0.0);
    } else {
        const double ang = atan2(sqrt(-disc), -(S + r3));
        u += 2.0 * r * cos(ang / 3.0);
    }
    const double v = sqrt(u * u + q), uv = u < 0.0 ? q / (v - u) : u + v, w = (uv - q) / (2.0 * v);
    return uv / (sqrt(uv + w * w) + w);
}
/* starting point of Newton's method; returns sig12 >= 0 when the line is short enough to be settled at once */
KQ double k_inverse_start(double sbet1, double cbet1, double dn1, double sbet2, double cbet2, double dn2, double lam12, double slam12, double clam12,
                       double* psalp1, double* pcalp1, double* psalp2, double* pcalp2, double* pdnm) {
    double salp1 = 0.0, calp1 = 0.0, salp2 = 0.0, calp2 = 0.0, dnm = 0.0;
    double sig12 = -1.0;
    const double sbet12 = sbet2 * cbet1 - cbet2 * sbet1, cbet12 = cbet2 * cbet1 + sbet2 * sbet1, sbet12a = sbet2 * cbet1 + cbet2 * sbet1;
    const int shortline = cbet12 >= 0.0 && sbet12 < 0.5 && cbet2 * lam12 < 0.5;
    double somg12, comg12;
    if (shortline) {
        double sbetm2 = k_sq(sbet1 + sbet2);
        sbetm2 /= sbetm2 + k_sq(cbet1 + cbet2);
        dnm = sqrt(1.0 + K_EP2 * sbetm2);
        const double omg12 = lam12 / (K_F1 * dnm);
        somg12 = sin(omg12);
        comg12 = cos(omg12);
    } else {
        somg12 = slam12;
        comg12 = clam12;
    }
    salp1 = cbet2 * somg12;
    calp1 = comg12 >= 0.0 ? sbet12 + cbet2 * sbet1 * k_sq(somg12) / (1.0 + comg12) : sbet12a - cbet2 * sbet1 * k_sq(somg12) / (1.0 - comg12);
    const double ssig12 = hypot(salp1, calp1), csig12 = sbet1 * sbet2 + cbet1 * cbet2 * comg12;
    if (shortline && ssig12 < K_ETOL2) {
        salp2 = cbet1 * somg12;
        calp2 = sbet12 - cbet1 * sbet2 * (comg12 >= 0.0 ? k_sq(somg12) / (1.0 + comg12) : 1.0 - comg12);
        k_norm2(&salp2, &calp2);
        sig12 = atan2(ssig12, csig12);
    } else if (fabs(K_N) > 0.1 || csig12 >= 0.0 || ssig12 >= 6.0 * fabs(K_N) * K_PI * k_sq(cbet1)) {
        /* nothing to do: zeroth-order spherical approximation is fine */
    } else {
        /* nearly antipodal points: scale lam12 and bet2 to x, y and solve the astroid problem */
        const double lam12x = atan2(-slam12, -clam12);
        const double k2 = k_sq(sbet1) * K_EP2, eps = k2 / (2.0 * (1.0 + sqrt(1.0 + k2)) + k2);
        const double lamscale = K_F * cbet1 * k_A3f(eps) * K_PI, betscale = lamscale * cbet1;
        const double x = lam12x / lamscale, y = sbet12a / betscale;
        if (y > -K_TOL1 && x > -1.0 - K_XTHRESH) {
            salp1 = fmin(1.0, -x);
            calp1 = -sqrt(1.0 - k_sq(salp1));
        } else {
            const double k = k_astroid(x, y);
            const double omg12a = lamscale * (-x * k / (1.0 + k));
            somg12 = sin(omg12a);
            comg12 = -cos(omg12a);
            salp1 = cbet2 * somg12;
            calp1 = sbet12a - cbet2 * sbet1 * k_sq(somg12) / (1.0 - comg12);
        }
    }
    if (!(salp1 <= 0.0)) {
        k_norm2(&salp1, &calp1);
    } else {
        salp1 = 1.0;
        calp1 = 0.0;
    }
    *psalp1 = salp1;
    *pcalp1 = calp1;
    *psalp2 = salp2;
    *pcalp2 = calp2;
    *pdnm = dnm;
    return sig12;
}
/* lambda12(alp1) - lam12 is what Newton's method drives to zero */
KQ double k_lambda12(double sbet1, double cbet1, double dn1, double sbet2, double cbet2, double dn2, double salp1, double calp1, double slam120,
                  double clam120, double* psalp2, double* pcalp2, double* psig12, double* pssig1, double* pcsig1, double* pssig2, double* pcsig2,
                  double* peps, double* pdomg12, int diffp, double* pdlam12) {
    if (sbet1 == 0.0 && calp1 == 0.0) calp1 = -K_TINY;
    const double salp0 = salp1 * cbet1, calp0 = hypot(calp1, salp1 * sbet1);
    double ssig1 = sbet1, csig1 = calp1 * cbet1;
    const double somg1 = salp0 * sbet1, comg1 = csig1;
    k_norm2(&ssig1, &csig1);
    const double salp2 = cbet2 != cbet1 ? salp0 / cbet2 : salp1;
    const double calp2 = (cbet2 != cbet1 || fabs(sbet2) != -sbet1)
                             ? sqrt(k_sq(calp1 * cbet1) + (cbet1 < -sbet1 ? (cbet2 - cbet1) * (cbet1 + cbet2) : (sbet1 - sbet2) * (sbet1 + sbet2))) / cbet2
                             : fabs(calp1);
    double ssig2 = sbet2, csig2 = calp2 * cbet2;
    const double somg2 = salp0 * sbet2, comg2 = csig2;
    k_norm2(&ssig2, &csig2);
    const double sig12 = atan2(fmax(0.0, csig1 * ssig2 - ssig1 * csig2), csig1 * csig2 + ssig1 * ssig2);
    const double somg12 = fmax(0.0, comg1 * somg2 - somg1 * comg2), comg12 = comg1 * comg2 + somg1 * somg2;
    const double eta = atan2(somg12 * clam120 - comg12 * slam120, comg12 * clam120 + somg12 * slam120);
    const double k2 = k_sq(calp0) * K_EP2, eps = k2 / (2.0 * (1.0 + sqrt(1.0 + k2)) + k2);
    double c3[6];
    k_C3f(eps, c3);
    const double B312 = k_sin_series(ssig2, csig2, c3, 5) - k_sin_series(ssig1, csig1, c3, 5);
    const double domg12 = -K_F * k_A3f(eps) * salp0 * (sig12 + B312);
    const double lam12 = eta + domg12;
    if (diffp) {
        if (calp2 == 0.0) {
            *pdlam12 = -2.0 * K_F1 * dn1 / sbet1;
        } else {
            double s12b, m12b, m0;
            k_lengths(eps, sig12, ssig1, csig1, dn1, ssig2, csig2, dn2, &s12b, &m12b, &m0);
            *pdlam12 = m12b * K_F1 / (calp2 * cbet2);
        }
    }
    *psalp2 = salp2;
    *pcalp2 = calp2;
    *psig12 = sig12;
    *pssig1 = ssig1;
    *pcsig1 = csig1;
    *pssig2 = ssig2;
    *pcsig2 = csig2;
    *peps = eps;
    *pdomg12 = domg12;
    return lam12;
}
/* sum of c[k] cos((2 k + 1) x), k = 0 .. N - 1 (Clenshaw) */
template <int N>
KQ double k_cos_series(double sinx, double cosx, const double* c) {
    const double ar = 2.0 * (cosx - sinx) * (cosx + sinx);
    double y0 = 0.0, y1 = 0.0;
    static_assert(N % 2 == 0, "even number of terms");
#pragma unroll
    for (int k = N; k > 0; k -= 2) {
        y1 = ar * y0 - y1 + c[k - 1];
        y0 = ar * y1 - y0 + c[k - 2];
    }
    return cosx * (y0 - y1);
}
/* the area series: c[l] = eps^l * (polynomial of order 5 - l in eps), whose coefficients are polynomials in n (constants here) */
KQ void k_C4f(double eps, double* c) {
    const double n = K_N;
    double m = eps;
    c[0] = ((((97.0 / 15015.0 * eps + (1088.0 * n + 156.0) / 45045.0) * eps + ((-224.0 * n - 4784.0) * n + 1573.0) / 45045.0) * eps +
             (((-10656.0 * n + 14144.0) * n - 4576.0) * n - 858.0) / 45045.0) * eps +
            ((((64.0 * n + 624.0) * n - 4576.0) * n + 6864.0) * n - 3003.0) / 15015.0) * eps +
           (((((100.0 * n + 208.0) * n + 572.0) * n + 3432.0) * n - 12012.0) * n + 30030.0) / 45045.0;
    c[1] = m * ((((1.0 / 9009.0 * eps + (-2944.0 * n + 468.0) / 135135.0) * eps + ((5792.0 * n + 1040.0) * n - 1287.0) / 135135.0) * eps +
                 (((5952.0 * n - 11648.0) * n + 9152.0) * n - 2574.0) / 135135.0) * eps +
                ((((-64.0 * n - 624.0) * n + 4576.0) * n - 6864.0) * n + 3003.0) / 135135.0);
    m *= eps;
    c[2] = m * (((8.0 / 10725.0 * eps + (1856.0 * n - 936.0) / 225225.0) * eps + ((-8448.0 * n + 4992.0) * n - 1144.0) / 225225.0) * eps +
                (((-1440.0 * n + 4160.0) * n - 4576.0) * n + 1716.0) / 225225.0);
    m *= eps;
    c[3] = m * ((-136.0 / 63063.0 * eps + (1024.0 * n - 208.0) / 105105.0) * eps + ((3584.0 * n - 3328.0) * n + 1144.0) / 315315.0);
    m *= eps;
    c[4] = m * (-128.0 / 135135.0 * eps + (-2560.0 * n + 832.0) / 405405.0);
    m *= eps;
    c[5] = m * (128.0 / 99099.0);
}
/* the reverted distance series of the direct problem */
KQ void k_C1pf(double eps, double* c) {
    const double e2 = eps * eps;
    double d = eps;
    c[1] = d * (e2 * (205.0 * e2 - 432.0) + 768.0) / 1536.0;
    d *= eps;
    c[2] = d * (e2 * (4005.0 * e2 - 4736.0) + 3840.0) / 12288.0;
    d *= eps;
    c[3] = d * (116.0 - 225.0 * e2) / 384.0;
    d *= eps;
    c[4] = d * (2695.0 - 7173.0 * e2) / 7680.0;
    d *= eps;
    c[5] = 3467.0 * d / 7680.0;
    d *= eps;
    c[6] = 38081.0 * d / 61440.0;
}
/* an angle into [-180, 180]; -180 only for a negative argument */
KQ double k_ang_normalize(double x) {
    const double y = remainder(x, 360.0);
    return fabs(y) == 180.0 ? copysign(180.0, x) : y;
}
/* atan2 in degrees, exact on the axes and the diagonals' multiples of 45 */
KQ double k_atan2d(double y, double x) {
    int q = 0;
    if (fabs(y) > fabs(x)) {
        const double t = x;
        x = y;
        y = t;
        q = 2;
    }
    if (signbit(x)) {
        x = -x;
        ++q;
    }
    double ang = atan2(y, x) / K_DEGREE;
    switch (q) {
        case 1: ang = copysign(180.0, y) - ang; break;
        case 2: ang = 90.0 - ang; break;
        case 3: ang = -90.0 + ang; break;
        default: break;
    }
    return ang;
}
/* +1 / -1 when the shortest edge from lon1 to lon2 crosses the prime meridian eastwards / westwards, else 0 */
KQ int transit(double lon1, double lon2) {
    double e;
    const double lon12 = k_ang_diff(lon1, lon2, &e);
    lon1 = k_ang_normalize(lon1);
    lon2 = k_ang_normalize(lon2);
    return lon12 > 0.0 && ((lon1 < 0.0 && lon2 >= 0.0) || (lon1 > 0.0 && lon2 == 0.0)) ? 1 : (lon12 < 0.0 && lon1 >= 0.0 && lon2 < 0.0 ? -1 : 0);
}
/* the inverse problem between (lon1, lat1) and (lon2, lat2), degrees.  AREA == false leaves S12 at 0 and skips its series.  A latitude
 * outside [-90, 90] or a NaN coordinate gives NaN in every field. */
template <bool AREA>
KQ Inverse inverse(double lon1, double lat1, double lon2, double lat2) {
    double lon12s;
    double lon12 = k_ang_diff(lon1, lon2, &lon12s);
    int lonsign = signbit(lon12) ? -1 : 1;
    lon12 *= lonsign;
    lon12s *= lonsign;
    const double lam12 = lon12 * K_DEGREE;
    double slam12, clam12;
    k_sincosd(lon12, &slam12, &clam12);
    lon12s = (180.0 - lon12) - lon12s;  /* the supplementary longitude difference */
    lat1 = k_ang_round(fabs(lat1) > 90.0 ? NAN : lat1);
    lat2 = k_ang_round(fabs(lat2) > 90.0 ? NAN : lat2);
    const int swapp = fabs(lat1) < fabs(lat2) || lat2 != lat2 ? -1 : 1;
    if (swapp < 0) {
        lonsign *= -1;
        const double t = lat1;
        lat1 = lat2;
        lat2 = t;
    }
    const int latsign = signbit(lat1) ? 1 : -1;
    lat1 *= latsign;
    lat2 *= latsign;
    double sbet1, cbet1, sbet2, cbet2;
    k_sincosd(lat1, &sbet1, &cbet1);
    sbet1 *= K_F1;
    k_norm2(&sbet1, &cbet1);
    cbet1 = fmax(K_TINY, cbet1);
    k_sincosd(lat2, &sbet2, &cbet2);
    sbet2 *= K_F1;
    k_norm2(&sbet2, &cbet2);
    cbet2 = fmax(K_TINY, cbet2);
    if (cbet1 < -sbet1) {
        if (cbet2 == cbet1) sbet2 = copysign(sbet1, sbet2);
    } else {
        if (fabs(sbet2) == -sbet1) cbet2 = cbet1;
    }
    const double dn1 = sqrt(1.0 + K_EP2 * k_sq(sbet1)), dn2 = sqrt(1.0 + K_EP2 * k_sq(sbet2));
    double s12x = 0.0, m12x = 0.0, sig12 = 0.0;
    double salp1 = 0.0, calp1 = 0.0, salp2 = 0.0, calp2 = 0.0;
    double omg12 = 0.0, somg12 = 2.0, comg12 = 0.0;  /* somg12 == 2: not set, take them from omg12 */
    int meridian = lat1 == -90.0 || slam12 == 0.0;
    if (meridian) {
        calp1 = clam12;  /* head to the target longitude */
        salp1 = slam12;
        calp2 = 1.0;  /* at the target we are heading north */
        salp2 = 0.0;
        const double ssig1 = sbet1, csig1 = calp1 * cbet1, ssig2 = sbet2, csig2 = calp2 * cbet2;
        sig12 = atan2(fmax(0.0, csig1 * ssig2 - ssig1 * csig2), csig1 * csig2 + ssig1 * ssig2);
        double m0;
        k_lengths(K_N, sig12, ssig1, csig1, dn1, ssig2, csig2, dn2, &s12x, &m12x, &m0);
        if (sig12 < 1.0 || m12x >= 0.0) {
            if (sig12 < 3.0 * K_TINY || (sig12 < K_TOL0 && (s12x < 0.0 || m12x < 0.0))) sig12 = m12x = s12x = 0.0;
            m12x *= K_B;
            s12x *= K_B;
        } else {
            meridian = 0;  /* m12 < 0: the prolate case, or the geodesic runs over a pole the long way */
        }
    }
    if (!meridian && sbet1 == 0.0 && lon12s >= K_F * 180.0) {
        calp1 = calp2 = 0.0;  /* along the equator */
        salp1 = salp2 = 1.0;
        s12x = K_A * lam12;
        sig12 = omg12 = lam12 / K_F1;
        m12x = K_B * sin(sig12);
    } else if (!meridian) {
        double dnm;
        sig12 = k_inverse_start(sbet1, cbet1, dn1, sbet2, cbet2, dn2, lam12, slam12, clam12, &salp1, &calp1, &salp2, &calp2, &dnm);
        if (sig12 >= 0.0) {
            s12x = sig12 * K_B * dnm;  /* short line */
            m12x = k_sq(dnm) * K_B * sin(sig12 / dnm);
            omg12 = lam12 / (K_F1 * dnm);
        } else {
            double ssig1 = 0.0, csig1 = 0.0, ssig2 = 0.0, csig2 = 0.0, eps = 0.0, domg12 = 0.0;
            double salp1a = K_TINY, calp1a = 1.0, salp1b = K_TINY, calp1b = -1.0;
            int tripn = 0, tripb = 0;
            for (int numit = 0; numit < K_MAXIT2; ++numit) {
                double dv = 0.0;
                const double v = k_lambda12(sbet1, cbet1, dn1, sbet2, cbet2, dn2, salp1, calp1, slam12, clam12, &salp2, &calp2, &sig12, &ssig1, &csig1,
                                            &ssig2, &csig2, &eps, &domg12, numit < K_MAXIT1, &dv);
                if (tripb || !(fabs(v) >= (tripn ? 8.0 : 1.0) * K_TOL0) || numit == K_MAXIT2 - 1) break;
                if (v > 0.0 && (numit > K_MAXIT1 || calp1 / salp1 > calp1b / salp1b)) {
                    salp1b = salp1;
                    calp1b = calp1;
                } else if (v < 0.0 && (numit > K_MAXIT1 || calp1 / salp1 < calp1a / salp1a)) {
                    salp1a = salp1;
                    calp1a = calp1;
                }
                if (numit < K_MAXIT1 && dv > 0.0) {
                    const double dalp1 = -v / dv;
                    if (fabs(dalp1) < K_PI) {
                        const double sdalp1 = sin(dalp1), cdalp1 = cos(dalp1), nsalp1 = salp1 * cdalp1 + calp1 * sdalp1;
                        if (nsalp1 > 0.0) {
                            calp1 = calp1 * cdalp1 - salp1 * sdalp1;
                            salp1 = nsalp1;
                            k_norm2(&salp1, &calp1);
                            tripn = fabs(v) <= 16.0 * K_TOL0;
                            continue;
                        }
                    }
                }
                salp1 = (salp1a + salp1b) / 2.0;
                calp1 = (calp1a + calp1b) / 2.0;
                k_norm2(&salp1, &calp1);
                tripn = 0;
                tripb = (fabs(salp1a - salp1) + (calp1a - calp1) < K_TOLB || fabs(salp1 - salp1b) + (calp1 - calp1b) < K_TOLB);
            }
            double m0;
            k_lengths(eps, sig12, ssig1, csig1, dn1, ssig2, csig2, dn2, &s12x, &m12x, &m0);
            m12x *= K_B;
            s12x *= K_B;
            if (AREA) {  /* omg12 = lam12 - domg12 */
                const double sdomg12 = sin(domg12), cdomg12 = cos(domg12);
                somg12 = slam12 * cdomg12 - clam12 * sdomg12;
                comg12 = clam12 * cdomg12 + slam12 * sdomg12;
            }
        }
    }
    Inverse r;
    r.s12 = 0.0 + s12x;
    r.m12 = 0.0 + m12x;
    r.S12 = 0.0;
    if (AREA) {
        const double salp0 = salp1 * cbet1, calp0 = hypot(calp1, salp1 * sbet1);  /* sin(alp1) cos(bet1) = sin(alp0) */
        double S12 = 0.0;
        if (calp0 != 0.0 && salp0 != 0.0) {
            double ssig1 = sbet1, csig1 = calp1 * cbet1, ssig2 = sbet2, csig2 = calp2 * cbet2;  /* tan(bet) = tan(sig) cos(alp) */
            const double k2 = k_sq(calp0) * K_EP2, eps = k2 / (2.0 * (1.0 + sqrt(1.0 + k2)) + k2);
            const double A4 = k_sq(K_A) * calp0 * salp0 * K_E2;
            k_norm2(&ssig1, &csig1);
            k_norm2(&ssig2, &csig2);
            double c4[6];
            k_C4f(eps, c4);
            const double B41 = k_cos_series<6>(ssig1, csig1, c4), B42 = k_cos_series<6>(ssig2, csig2, c4);
            S12 = A4 * (B42 - B41);
        }
        if (!meridian && somg12 == 2.0) {
            somg12 = sin(omg12);
            comg12 = cos(omg12);
        }
        double alp12;
        if (!meridian && comg12 > -0.7071 && sbet2 - sbet1 < 1.75) {
            /* the spherical excess: tan(Gamma / 2) = tan(omg12 / 2) (tan(bet1 / 2) + tan(bet2 / 2)) / (1 + tan(bet1 / 2) tan(bet2 / 2)),
             * with tan(x / 2) = sin(x) / (1 + cos(x)): no cancellation for a short edge */
            const double domg12 = 1.0 + comg12, dbet1 = 1.0 + cbet1, dbet2 = 1.0 + cbet2;
            alp12 = 2.0 * atan2(somg12 * (sbet1 * dbet2 + sbet2 * dbet1), domg12 * (sbet1 * sbet2 + dbet1 * dbet2));
        } else {
            double salp12 = salp2 * calp1 - calp2 * salp1, calp12 = calp2 * calp1 + salp2 * salp1;  /* alp2 - alp1 */
            if (salp12 == 0.0 && calp12 < 0.0) {  /* alp1 = +-180, alp2 = 0: the sign of the zero decides */
                salp12 = K_TINY * calp1;
                calp12 = -1.0;
            }
            alp12 = atan2(salp12, calp12);
        }
        S12 += K_C2 * alp12;
        S12 *= swapp * lonsign * latsign;
        r.S12 = 0.0 + S12;
    }
    if (swapp < 0) {
        double t = salp1;
        salp1 = salp2;
        salp2 = t;
        t = calp1;
        calp1 = calp2;
        calp2 = t;
    }
    salp1 *= swapp * lonsign;
    calp1 *= swapp * latsign;
    salp2 *= swapp * lonsign;
    calp2 *= swapp * latsign;
    r.azi1 = k_atan2d(salp1, calp1);
    r.azi2 = k_atan2d(salp2, calp2);
    if (r.s12 != r.s12) r.azi1 = r.azi2 = r.m12 = r.S12 = NAN;  /* a NaN input or a latitude out of range: every field */
    return r;
}
/* the direct problem: from (lon1, lat1) along azimuth azi1 (degrees) for s12 metres (negative: backwards) */
KQ Direct direct(double lon1, double lat1, double azi1, double s12) {
    double salp1, calp1, sbet1, cbet1;
    k_sincosd(k_ang_round(k_ang_normalize(azi1)), &salp1, &calp1);
    k_sincosd(k_ang_round(fabs(lat1) > 90.0 ? NAN : lat1), &sbet1, &cbet1);
    sbet1 *= K_F1;
    k_norm2(&sbet1, &cbet1);
    cbet1 = fmax(K_TINY, cbet1);
    const double salp0 = salp1 * cbet1, calp0 = hypot(calp1, salp1 * sbet1);
    double ssig1 = sbet1, csig1 = (sbet1 != 0.0 || calp1 != 0.0) ? cbet1 * calp1 : 1.0;
    const double somg1 = salp0 * sbet1, comg1 = csig1;
    k_norm2(&ssig1, &csig1);
    const double k2 = k_sq(calp0) * K_EP2, eps = k2 / (2.0 * (1.0 + sqrt(1.0 + k2)) + k2);
    const double A1m1 = k_A1m1f(eps);
    double c1[7], c1p[7], c3[6];
    k_C1f(eps, c1);
    const double B11 = k_sin_series(ssig1, csig1, c1, 6);
    const double sB = sin(B11), cB = cos(B11);
    const double stau1 = ssig1 * cB + csig1 * sB, ctau1 = csig1 * cB - ssig1 * sB;  /* tau1 = sig1 + B11 */
    k_C1pf(eps, c1p);
    const double A3c = -K_F * salp0 * k_A3f(eps);
    k_C3f(eps, c3);
    const double B31 = k_sin_series(ssig1, csig1, c3, 5);
    const double tau12 = s12 / (K_B * (1.0 + A1m1));
    const double st = sin(tau12), ct = cos(tau12);
    const double B12 = -k_sin_series(stau1 * ct + ctau1 * st, ctau1 * ct - stau1 * st, c1p, 6);
    const double sig12 = tau12 - (B12 - B11);
    const double ssig12 = sin(sig12), csig12 = cos(sig12);
    const double ssig2 = ssig1 * csig12 + csig1 * ssig12;
    double csig2 = csig1 * csig12 - ssig1 * ssig12;
    const double sbet2 = calp0 * ssig2;
    double cbet2 = hypot(salp0, calp0 * csig2);
    if (cbet2 == 0.0) cbet2 = csig2 = K_TINY;  /* a pole */
    const double salp2 = salp0, calp2 = calp0 * csig2;
    const double somg2 = salp0 * ssig2, comg2 = csig2;
    const double omg12 = atan2(somg2 * comg1 - comg2 * somg1, comg2 * comg1 + somg2 * somg1);
    const double lam12 = omg12 + A3c * (sig12 + (k_sin_series(ssig2, csig2, c3, 5) - B31));
    Direct r;
    r.lon2 = k_ang_normalize(k_ang_normalize(lon1) + k_ang_normalize(lam12 / K_DEGREE));
    r.lat2 = k_atan2d(sbet2, K_F1 * cbet2);
    r.azi2 = k_atan2d(salp2, calp2);
    if (r.lat2 != r.lat2 || r.lon2 != r.lon2) r.lon2 = r.lat2 = r.azi2 = NAN;
    return r;
}

/* ---- the two other methods of gpk_geodesic_length: metres between (lon1, lat1) and (lon2, lat2), degrees ------------------------- */
// geo 0.27 haversine_distance.rs: mean earth radius 6371008.8 m (IUGG), the half-angle formula
KQ double haversine_m(double lon1, double lat1, double lon2, double lat2) {
    const double rad = 0.017453292519943295;  // pi / 180 (f64::to_radians multiplies by this constant)
    const double t1 = lat1 * rad, t2 = lat2 * rad;
    const double dt = (lat2 - lat1) * rad, dl = (lon2 - lon1) * rad;
    const double sh = sin(dt / 2.0), sl = sin(dl / 2.0);
    const double a = sh * sh + cos(t1) * cos(t2) * (sl * sl);
    return 6371008.8 * (2.0 * asin(sqrt(a)));
}
// geo 0.27 vincenty_distance.rs (Vincenty's inverse formula on WGS84, at most 100 iterations, |d lambda| <= 1e-12):
// NaN where upstream returns Err(FailedToConvergeError) (nearly antipodal points)
KQ double vincenty_m(double lon1, double lat1, double lon2, double lat2) {
    const double rad = 0.017453292519943295;
    const double a = 6378137.0, b = 6356752.314245, f = 1.0 / 298.257223563;
    const double L = (lon2 - lon1) * rad;
    const double U1 = atan((1.0 - f) * tan(lat1 * rad)), U2 = atan((1.0 - f) * tan(lat2 * rad));
    const double sU1 = sin(U1), cU1 = cos(U1), sU2 = sin(U2), cU2 = cos(U2);
    double lam = L, lam_p, sS = 0, cS = 0, sig = 0, c2A = 0, c2SM = 0;
    int it = 100;
    for (;;) {
        const double sl = sin(lam), cl = cos(lam);
        const double t0 = cU2 * sl, t1 = cU1 * sU2 - sU1 * cU2 * cl;
        sS = sqrt(t0 * t0 + t1 * t1);
        if (sS == 0.0) return (lon1 == lon2 && lat1 == lat2) ? 0.0 : NAN;  // coincident points: 0
        cS = sU1 * sU2 + cU1 * cU2 * cl;
        sig = atan2(sS, cS);
        const double sA = cU1 * cU2 * sl / sS;
        c2A = 1.0 - sA * sA;
        c2SM = c2A == 0.0 ? 0.0 : cS - 2.0 * sU1 * sU2 / c2A;  // equatorial line: cos^2 alpha = 0
        const double C = f / 16.0 * c2A * (4.0 + f * (4.0 - 3.0 * c2A));
        lam_p = lam;
        lam = L + (1.0 - C) * f * sA * (sig + C * sS * (c2SM + C * cS * (-1.0 + 2.0 * c2SM * c2SM)));
        if (fabs(lam - lam_p) <= 1e-12) break;
        if (--it == 0) return NAN;
    }
    const double uSq = c2A * (a * a - b * b) / (b * b);
    const double A = 1.0 + uSq / 16384.0 * (4096.0 + uSq * (-768.0 + uSq * (320.0 - 175.0 * uSq)));
    const double B = uSq / 1024.0 * (256.0 + uSq * (-128.0 + uSq * (74.0 - 47.0 * uSq)));
    const double dS = B * sS * (c2SM + B / 4.0 * (cS * (-1.0 + 2.0 * c2SM * c2SM) - B / 6.0 * c2SM * (-3.0 + 4.0 * sS * sS) * (-3.0 + 4.0 * c2SM * c2SM)));
    return b * A * (sig - dS);
}

/* ---- error-free sums: the area of a ring is a sum of terms up to 1e13 m^2 that cancel ------------------------------------------ */
struct Sum2 {
    double hi, lo;
};
KQ Sum2 sum2_add(Sum2 a, double v) {  /* (hi, lo) + v; hi + lo is the sum to about 2^-104 relative */
    const double s = a.hi + v, bb = s - a.hi, e = (a.hi - (s - bb)) + (v - bb);
    const double lo = a.lo + e, hi = s + lo;
    Sum2 r;
    r.hi = hi;
    r.lo = lo - (hi - s);
    return r;
}
KQ Sum2 sum2_join(Sum2 a, Sum2 b) { return sum2_add(sum2_add(a, b.hi), b.lo); }
/* a ring's signed area from the sum of its edges' S12 and the sum of their transit counts: the sum is the CLOCKWISE area modulo half the
 * ellipsoid; the result is the area to the left of the direction of travel (counter-clockwise positive) in (-AREA0 / 2, AREA0 / 2] */
KQ double ring_area(Sum2 a, int crossings) {
    Sum2 z;
    z.hi = remainder(a.hi, AREA0);
    z.lo = 0.0;
    a = sum2_add(z, a.lo);
    if (crossings & 1) a = sum2_add(a, (a.hi < 0.0 ? 1.0 : -1.0) * (AREA0 / 2.0));
    a.hi = -a.hi;
    a.lo = -a.lo;
    if (a.hi > AREA0 / 2.0) a = sum2_add(a, -AREA0);
    else if (a.hi <= -AREA0 / 2.0) a = sum2_add(a, AREA0);
    return 0.0 + a.hi;
}
#undef KQ
#undef K_A
#undef K_F
#undef K_F1
#undef K_E2
#undef K_EP2
#undef K_N
#undef K_B
#undef K_PI
#undef K_DEGREE
#undef K_TINY
#undef K_TOL0
#undef K_TOL1
#undef K_TOL2
#undef K_TOLB
#undef K_XTHRESH
#undef K_ETOL2
#undef K_MAXIT1
#undef K_MAXIT2
#undef K_C2

}  // namespace geodesic
}  // namespace gpk
