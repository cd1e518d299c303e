// geodesic_host_driver.cpp — runs csrc/gpk_geodesic.h on the CPU over the mp fixture (tests/test_geodesic_host.py builds it twice with
// the host compiler: plain, and with -fsanitize=address,undefined).  A stand-alone program:
//   geodesic_host_driver in.bin out.bin
// in.bin   int64 n_edges, n_direct, n_rings, n_ring_coords; edge_xy[n_edges][4]; edge_expected[n_edges][5] (s12, azi1, azi2, m12, S12);
//          edge_regime[n_edges] (int32); direct_in[n_direct][4]; direct_expected[n_direct][3]; ring_off[n_rings + 1] (int32);
//          ring_regime[n_rings] (int32); ring_xy[n_ring_coords][2]; ring_expected[n_rings][2] (signed area, perimeter)
// out.bin  edges[n_edges][7] (s12, azi1, azi2, m12, S12, then the haversine and the Vincenty metres of the same edge); direct[n_direct][3];
//          rings[n_rings][2] — what the header computed
// stdout   the worst error per regime: distances in metres, azimuths as |d azi| * |m12| in metres, areas in m^2 (per edge for rings)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_geodesic.h"

namespace geo = gpk::geodesic;

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static double wrap(double d) { return std::remainder(d, 360.0); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t h[4];
    if (fread(h, sizeof(int64_t), 4, f) != 4) return 4;
    const size_t ne = (size_t)h[0], nd = (size_t)h[1], nr = (size_t)h[2], nc = (size_t)h[3];
    std::vector<double> exy, eexp, din, dexp, rxy, rexp;
    std::vector<int32_t> ereg, roff, rreg;
    if (!read_n(f, exy, 4 * ne) || !read_n(f, eexp, 5 * ne) || !read_n(f, ereg, ne) || !read_n(f, din, 4 * nd) || !read_n(f, dexp, 3 * nd) ||
        !read_n(f, roff, nr + 1) || !read_n(f, rreg, nr) || !read_n(f, rxy, 2 * nc) || !read_n(f, rexp, 2 * nr))
        return 5;
    fclose(f);
    std::vector<double> eout(7 * ne), dout(3 * nd), rout(2 * nr);
    constexpr int MAXREG = 16;
    double w_s[MAXREG] = {0}, w_azi[MAXREG] = {0}, w_S[MAXREG] = {0}, w_plain[MAXREG] = {0};
    for (size_t i = 0; i < ne; ++i) {
        const double* p = &exy[4 * i];
        const geo::Inverse r = geo::inverse<true>(p[0], p[1], p[2], p[3]);
        const geo::Inverse r0 = geo::inverse<false>(p[0], p[1], p[2], p[3]);
        double* o = &eout[7 * i];
        o[0] = r.s12, o[1] = r.azi1, o[2] = r.azi2, o[3] = r.m12, o[4] = r.S12;
        o[5] = geo::haversine_m(p[0], p[1], p[2], p[3]), o[6] = geo::vincenty_m(p[0], p[1], p[2], p[3]);
        const double* x = &eexp[5 * i];
        const int k = ereg[i] & (MAXREG - 1);
        w_s[k] = std::max(w_s[k], std::fabs(r.s12 - x[0]) / (1e-9 * std::fabs(x[0]) + 2e-8));  // in units of the project's Karney bound
        const double m = std::fabs(x[3]) * (M_PI / 180.0);
        w_azi[k] = std::max(w_azi[k], std::max(std::fabs(wrap(r.azi1 - x[1])), std::fabs(wrap(r.azi2 - x[2]))) * m);
        if (x[4] == x[4]) w_S[k] = std::max(w_S[k], std::fabs(r.S12 - x[4]));
        w_plain[k] = std::max(w_plain[k], (r0.s12 == r.s12 && r0.azi1 == r.azi1 && r0.azi2 == r.azi2 && r0.S12 == 0.0) ? 0.0 : 1.0);
    }
    for (int k = 0; k < MAXREG; ++k)
        if (std::count(ereg.begin(), ereg.end(), k))
            printf("edge regime %d: s12 %.3e of the bound, azimuth %.3e m, S12 %.3e m^2, area-free instance differs: %.0f\n", k, w_s[k], w_azi[k], w_S[k],
                   w_plain[k]);
    double w_d = 0.0, w_dazi = 0.0;
    for (size_t i = 0; i < nd; ++i) {
        const double* p = &din[4 * i];
        const geo::Direct r = geo::direct(p[0], p[1], p[2], p[3]);
        double* o = &dout[3 * i];
        o[0] = r.lon2, o[1] = r.lat2, o[2] = r.azi2;
        const double* x = &dexp[3 * i];
        w_d = std::max(w_d, geo::inverse<false>(r.lon2, r.lat2, x[0], x[1]).s12);
        w_dazi = std::max(w_dazi, std::fabs(wrap(r.azi2 - x[2])));
    }
    printf("direct: %.3e m to the reference point, azimuth %.3e degrees\n", w_d, w_dazi);
    double w_a[MAXREG] = {0}, w_arel[MAXREG] = {0}, w_p[MAXREG] = {0};
    for (size_t i = 0; i < nr; ++i) {
        geo::Sum2 a{0.0, 0.0};
        double per = 0.0;
        int crossings = 0;
        for (int32_t c = roff[i]; c + 1 < roff[i + 1]; ++c) {
            const geo::Inverse r = geo::inverse<true>(rxy[2 * c], rxy[2 * c + 1], rxy[2 * c + 2], rxy[2 * c + 3]);
            a = geo::sum2_add(a, r.S12);
            per += r.s12;
            crossings += geo::transit(rxy[2 * c], rxy[2 * c + 2]);
        }
        rout[2 * i] = geo::ring_area(a, crossings);
        rout[2 * i + 1] = per;
        const int k = rreg[i] & (MAXREG - 1);
        const int edges = std::max(1, roff[i + 1] - roff[i] - 1);
        const double err = std::fabs(rout[2 * i] - rexp[2 * i]);
        w_a[k] = std::max(w_a[k], err / edges);
        w_arel[k] = std::max(w_arel[k], err / std::max(1e-300, std::fabs(rexp[2 * i])));
        w_p[k] = std::max(w_p[k], std::fabs(per - rexp[2 * i + 1]) / (1e-9 * rexp[2 * i + 1] + 2e-8 * edges));
    }
    for (int k = 0; k < MAXREG; ++k)
        if (std::count(rreg.begin(), rreg.end(), k))
            printf("ring regime %d: area %.3e m^2 per edge (%.3e relative), perimeter %.3e of the bound\n", k, w_a[k], w_arel[k], w_p[k]);
    f = fopen(argv[2], "wb");
    if (!f) return 6;
    fwrite(eout.data(), sizeof(double), eout.size(), f);
    fwrite(dout.data(), sizeof(double), dout.size(), f);
    fwrite(rout.data(), sizeof(double), rout.size(), f);
    fclose(f);
    return 0;
}
