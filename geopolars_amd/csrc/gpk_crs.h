// gpk_crs.h — analytic reprojection between a closed set of systems on the WGS84 ellipsoid:
//   geographic lon/lat degrees (EPSG:4326 in x = lon order), spherical Web Mercator (3857), ellipsoidal Mercator (3395) and
//   transverse Mercator with UTM parameters (326zz / 327zz).
// Plain C++: no HIP type appears here, so a host program can include the file and run the very code the kernel runs
// (tests/crs_host_driver.cpp).  Under hipcc every function is __host__ __device__.
//
// Transverse Mercator is the Krueger series to n^6 in the form of Karney, "Transverse Mercator with an accuracy of a few
// nanometers", J. Geodesy 85 (2011), eqs. 7-11, 25-36 — what PROJ's etmerc and GeographicLib evaluate.  Each transform runs
// source -> (sin phi, cos phi, longitude in degrees) -> destination; the geographic intermediate lives in registers.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GPK_CRS_FN __host__ __device__ inline
#else
#define GPK_CRS_FN inline
#endif

enum { GPK_CRS_GEOG = 0, GPK_CRS_WEBMERC = 1, GPK_CRS_MERC = 2, GPK_CRS_TMERC = 3 };

#define GPK_CRS_A 6378137.0
#define GPK_CRS_E 0.0818191908426214943348     /* first eccentricity, 1/f = 298.257223563 */
#define GPK_CRS_E2M 0.993305620009858683004    /* 1 - e^2 */
#define GPK_CRS_INV_E2M 1.00673949674227643495 /* 1 / (1 - e^2) */
#define GPK_CRS_N 0.00167922038638370469510    /* third flattening f / (2 - f) */
#define GPK_CRS_K0 0.9996
#define GPK_CRS_DEG 0.0174532925199432957692   /* radians per degree */
#define GPK_CRS_RAD 57.2957795130823208768     /* degrees per radian */
#define GPK_CRS_COS90 6.123233995736766e-17    /* cos of the double nearest pi/2: the floor of cos(lat) on the way into a transverse Mercator */
#define GPK_CRS_NEWTON 3                       /* fixed iteration count of the tau' -> tau solve */

// everything a (source, destination) pair needs, computed once per call on the host and passed by value as a kernel argument
struct gpk_crs_params {
    double alp[6], bet[6];  // Krueger series, forward and inverse
    double k0A, inv_k0A;    // k0 * rectifying radius, and its reciprocal
    double s_lon0, s_fe, s_fn;  // source: central meridian (degrees), false easting / northing (transverse Mercator only)
    double d_lon0, d_fe, d_fn;  // destination
};

// ---- host side: the supported codes and the series coefficients ------------------------------------------------------------
// kind of an EPSG code (-1: not supported) and its transverse-Mercator parameters
inline int gpk_crs_describe(int32_t epsg, double* lon0, double* fe, double* fn) {
    *lon0 = 0.0, *fe = 0.0, *fn = 0.0;
    if (epsg == 4326) return GPK_CRS_GEOG;
    if (epsg == 3857) return GPK_CRS_WEBMERC;
    if (epsg == 3395) return GPK_CRS_MERC;
    const bool north = epsg >= 32601 && epsg <= 32660, south = epsg >= 32701 && epsg <= 32760;
    if (!north && !south) return -1;
    const int zone = epsg - (north ? 32600 : 32700);
    *lon0 = 6.0 * zone - 183.0;
    *fe = 500000.0;
    *fn = north ? 0.0 : 10000000.0;
    return GPK_CRS_TMERC;
}

// false when a code is not supported
inline bool gpk_crs_make_params(int32_t src_epsg, int32_t dst_epsg, gpk_crs_params* P, int* src_kind, int* dst_kind) {
    *src_kind = gpk_crs_describe(src_epsg, &P->s_lon0, &P->s_fe, &P->s_fn);
    *dst_kind = gpk_crs_describe(dst_epsg, &P->d_lon0, &P->d_fe, &P->d_fn);
    if (*src_kind < 0 || *dst_kind < 0) return false;
    const double n = GPK_CRS_N, n2 = n * n, n3 = n2 * n, n4 = n2 * n2, n5 = n4 * n, n6 = n3 * n3;
    // Karney (2011) eqs. 35 and 36
    P->alp[0] = n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800;
    P->alp[1] = 13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360;
    P->alp[2] = 61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440;
    P->alp[3] = 49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600;
    P->alp[4] = 34729 * n5 / 80640 - 3418889 * n6 / 1995840;
    P->alp[5] = 212378941 * n6 / 319334400;
    P->bet[0] = n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800;
    P->bet[1] = n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720;
    P->bet[2] = 17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720;
    P->bet[3] = 4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600;
    P->bet[4] = 4583 * n5 / 161280 - 108847 * n6 / 3991680;
    P->bet[5] = 20648693 * n6 / 638668800;
    const double A = GPK_CRS_A / (1 + n) * (1 + n2 / 4 + n4 / 64 + n6 / 256);  // rectifying radius, eq. 14
    P->k0A = GPK_CRS_K0 * A;
    P->inv_k0A = 1.0 / P->k0A;
    return true;
}

// ---- device math ---------------------------------------------------------------------------------------------------------------
// longitude difference into [-180, 180]; +-180 stay what they are
GPK_CRS_FN double gpk_crs_wrap180(double d) {
    d = d > 180.0 ? d - 360.0 : (d < -180.0 ? d + 360.0 : d);
    if (!(fabs(d) <= 180.0)) d = remainder(d, 360.0);  // more than a turn and a half away (rare); NaN stays NaN
    return d;
}

// sigma = sinh(e * atanh(e * s)), s = sin(phi).  |e s| <= 0.082 and |e atanh(e s)| <= 0.0068: both functions are their Taylor
// series, truncated below 2^-60 relative — no logarithm, no exponential, no division
GPK_CRS_FN double gpk_crs_sigma(double s) {
    const double x = GPK_CRS_E * s, x2 = x * x;
    double p = 1.0 / 17.0;
    p = fma(p, x2, 1.0 / 15.0);
    p = fma(p, x2, 1.0 / 13.0);
    p = fma(p, x2, 1.0 / 11.0);
    p = fma(p, x2, 1.0 / 9.0);
    p = fma(p, x2, 1.0 / 7.0);
    p = fma(p, x2, 1.0 / 5.0);
    p = fma(p, x2, 1.0 / 3.0);
    p = fma(p, x2, 1.0);
    const double t = GPK_CRS_E * (x * p), t2 = t * t;
    double q = 1.0 / 362880.0;
    q = fma(q, t2, 1.0 / 5040.0);
    q = fma(q, t2, 1.0 / 120.0);
    q = fma(q, t2, 1.0 / 6.0);
    q = fma(q, t2, 1.0);
    return t * q;
}

// tau' = tan of the conformal latitude from sin, 1/cos and tan of the geographic one (Karney eqs. 7-9)
GPK_CRS_FN double gpk_crs_taup(double s, double tau, double tau1) {
    const double sig = gpk_crs_sigma(s);
    return tau * sqrt(1.0 + sig * sig) - sig * tau1;
}

// tau from tau' by Newton (Karney eqs. 19-21).  The start tau' / (1 - e^2) is within 2e-5 relative everywhere, every step
// squares that: the count is fixed, there is no data-dependent exit
GPK_CRS_FN double gpk_crs_tau_from_taup(double taup) {
    double tau = taup * GPK_CRS_INV_E2M;
    for (int k = 0; k < GPK_CRS_NEWTON; ++k) {
        const double tau1 = sqrt(1.0 + tau * tau), r = 1.0 / tau1;
        const double tpa = gpk_crs_taup(tau * r, tau, tau1);
        const double dtau = (taup - tpa) * (1.0 + GPK_CRS_E2M * (tau * tau)) * r / (GPK_CRS_E2M * sqrt(1.0 + tpa * tpa));
        tau += dtau;
    }
    return tau;
}

GPK_CRS_FN double gpk_crs_sinh(double x) {
    const double e = exp(x);
    return 0.5 * (e - 1.0 / e);
}

// sum_j c[j-1] sin(2 j zeta), zeta = xi + i eta, by Clenshaw's recurrence in real arithmetic from sin / cos of 2 xi and
// sinh / cosh of 2 eta: re is the sum's real part (the xi correction), im its imaginary part (the eta correction)
GPK_CRS_FN void gpk_crs_clenshaw(const double* c, double s2, double c2, double sh2, double ch2, double* re, double* im) {
    const double ar = 2.0 * c2 * ch2, ai = -2.0 * s2 * sh2;  // 2 cos(2 zeta)
    double y0r = c[5], y0i = 0.0, y1r = 0.0, y1i = 0.0;
#pragma unroll
    for (int j = 4; j >= 0; --j) {
        const double tr = fma(ar, y0r, -(ai * y0i)) - y1r + c[j];
        const double ti = fma(ar, y0i, ai * y0r) - y1i;
        y1r = y0r, y1i = y0i, y0r = tr, y0i = ti;
    }
    const double zr = s2 * ch2, zi = c2 * sh2;  // sin(2 zeta)
    *re = zr * y0r - zi * y0i;
    *im = zr * y0i + zi * y0r;
}

// the geographic intermediate: sin and cos of the latitude (cos >= 0; exactly 0 at a pole) and the longitude in degrees
struct gpk_crs_geo {
    double s, c, lon;
};

template <int SK>
GPK_CRS_FN bool gpk_crs_to_geo(const gpk_crs_params& P, double x, double y, gpk_crs_geo* g) {
    if (!(fabs(x) <= 1.79769313486231570815e308 && fabs(y) <= 1.79769313486231570815e308)) return false;  // NaN or infinite
    double tau;
    if (SK == GPK_CRS_GEOG) {
        if (fabs(y) > 90.0) return false;
        sincos(y * GPK_CRS_DEG, &g->s, &g->c);
        if (fabs(y) == 90.0) g->s = y < 0 ? -1.0 : 1.0, g->c = 0.0;
        g->lon = x;
        return true;
    } else if (SK == GPK_CRS_WEBMERC) {
        tau = gpk_crs_sinh(y * (1.0 / GPK_CRS_A));
        g->lon = x * (GPK_CRS_RAD / GPK_CRS_A);
    } else if (SK == GPK_CRS_MERC) {
        tau = gpk_crs_tau_from_taup(gpk_crs_sinh(y * (1.0 / GPK_CRS_A)));
        g->lon = x * (GPK_CRS_RAD / GPK_CRS_A);
    } else {
        const double xi = (y - P.s_fn) * P.inv_k0A, eta = (x - P.s_fe) * P.inv_k0A;
        double s2, c2;
        sincos(2.0 * xi, &s2, &c2);
        const double e2 = exp(2.0 * eta), ie2 = 1.0 / e2;
        double dxi, deta;
        gpk_crs_clenshaw(P.bet, s2, c2, 0.5 * (e2 - ie2), 0.5 * (e2 + ie2), &dxi, &deta);
        double sx, cx;
        sincos(xi - dxi, &sx, &cx);
        const double sh = gpk_crs_sinh(eta - deta);
        const double r2 = sh * sh + cx * cx;
        g->lon = P.s_lon0 + atan2(sh, cx) * GPK_CRS_RAD;
        if (!(r2 > 0.0)) {  // the pole itself
            g->s = sx < 0 ? -1.0 : 1.0, g->c = 0.0;
            return true;
        }
        tau = gpk_crs_tau_from_taup(sx / sqrt(r2));
    }
    g->c = 1.0 / sqrt(1.0 + tau * tau);
    g->s = tau * g->c;
    return true;
}

template <int DK>
GPK_CRS_FN bool gpk_crs_from_geo(const gpk_crs_params& P, const gpk_crs_geo& g, double* ox, double* oy) {
    if (DK == GPK_CRS_GEOG) {
        *ox = gpk_crs_wrap180(g.lon);
        *oy = atan2(g.s, g.c) * GPK_CRS_RAD;
    } else if (DK == GPK_CRS_WEBMERC) {
        *ox = gpk_crs_wrap180(g.lon) * (GPK_CRS_A * GPK_CRS_DEG);
        *oy = GPK_CRS_A * asinh(g.s / g.c);
    } else if (DK == GPK_CRS_MERC) {
        const double rc = 1.0 / g.c;
        *ox = gpk_crs_wrap180(g.lon) * (GPK_CRS_A * GPK_CRS_DEG);
        *oy = GPK_CRS_A * asinh(gpk_crs_taup(g.s, g.s * rc, rc));
    } else {
        const double dl = gpk_crs_wrap180(g.lon - P.d_lon0);
        if (!(fabs(dl) < 90.0)) return false;
        const double rc = 1.0 / (g.c > GPK_CRS_COS90 ? g.c : GPK_CRS_COS90);
        const double taup = gpk_crs_taup(g.s, g.s * rc, rc);
        double sl, cl;
        sincos(dl * GPK_CRS_DEG, &sl, &cl);
        // xi' = atan2(tau', cos lam), eta' = asinh(sin lam / hypot(tau', cos lam)) (Karney eq. 10); the double-angle
        // functions the series needs follow from tau', cos lam and sin lam without going through xi' and eta'
        const double inv = 1.0 / (taup * taup + cl * cl);
        const double s2 = 2.0 * taup * cl * inv, c2 = (cl - taup) * (cl + taup) * inv;
        const double sh2 = 2.0 * sl * sqrt(1.0 + taup * taup) * inv, ch2 = 1.0 + 2.0 * (sl * sl) * inv;
        double dxi, deta;
        gpk_crs_clenshaw(P.alp, s2, c2, sh2, ch2, &dxi, &deta);
        const double xi = atan2(taup, cl) + dxi, eta = asinh(sl * sqrt(inv)) + deta;
        *ox = P.d_fe + P.k0A * eta;
        *oy = P.d_fn + P.k0A * xi;
    }
    return fabs(*ox) <= 1.79769313486231570815e308 && fabs(*oy) <= 1.79769313486231570815e308;
}

// one coordinate; false (and NaN, NaN) when it fails: a non-finite input, a geographic latitude beyond +-90, a transverse
// Mercator destination 90 degrees or more from its central meridian, a non-finite result
template <int SK, int DK>
GPK_CRS_FN bool gpk_crs_transform(const gpk_crs_params& P, double x, double y, double* ox, double* oy) {
    gpk_crs_geo g;
    if (gpk_crs_to_geo<SK>(P, x, y, &g) && gpk_crs_from_geo<DK>(P, g, ox, oy)) return true;
    *ox = *oy = NAN;
    return false;
}

// the instance table, for callers that learn the kinds at run time (the kernel launcher and the host driver).  F is called as
// f.template operator()<SK, DK>(); same kind -> same kind exists for the transverse Mercator only (zone to zone)
template <typename F>
inline bool gpk_crs_dispatch(int sk, int dk, F&& f) {
#define GPK_CRS_CASE(S, D) \
    case (S) * 4 + (D): f.template operator()<S, D>(); return true;
    switch (sk * 4 + dk) {
        GPK_CRS_CASE(0, 1) GPK_CRS_CASE(0, 2) GPK_CRS_CASE(0, 3)
        GPK_CRS_CASE(1, 0) GPK_CRS_CASE(1, 2) GPK_CRS_CASE(1, 3)
        GPK_CRS_CASE(2, 0) GPK_CRS_CASE(2, 1) GPK_CRS_CASE(2, 3)
        GPK_CRS_CASE(3, 0) GPK_CRS_CASE(3, 1) GPK_CRS_CASE(3, 2) GPK_CRS_CASE(3, 3)
    }
#undef GPK_CRS_CASE
    return false;
}
