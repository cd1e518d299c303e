// The seed walk of gpk_nearest_join_any (geopolars_amd/csrc/gpk_nearwalk.h) on the CPU: a stand-alone program, no GPU.  For every case it
// builds a bbox grid directory on the host with the header's own cell function (a right row is listed in every cell its closed box
// meets, ids ascending within a cell — the shape of the library's directory), runs the walk for a few hundred left boxes and compares
// the seed with the brute-force answer: the lowest usable right row among those whose box is nearest, within max_d + margin.  The box
// distances must agree bit for bit.  Coordinates are multiples of 1/8, so equal box distances (ties) are common.
// Output: one line per case, "<name> <left boxes> <seeded> <mismatches>"; exit status 1 when any case has a mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gpk_nearwalk.h"

using namespace gpk;

namespace {

struct Rng {  // (splitmix64: the same numbers with every compiler)
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    // a multiple of 1/8 in [lo, hi]
    double eighth(double lo, double hi) {
        const int64_t a = (int64_t)(lo * 8.0), b = (int64_t)(hi * 8.0);
        return (double)(a + (int64_t)(next() % (uint64_t)(b - a + 1))) / 8.0;
    }
};

struct HostDir {
    std::vector<int> cell_off, items;
    std::vector<nw::Box> boxes;
    std::vector<char> valid;
    int cell_begin(int c) const { return cell_off[(size_t)c]; }
    int cell_end(int c) const { return cell_off[(size_t)c + 1]; }
    uint32_t item(int k) const { return (uint32_t)items[(size_t)k]; }
    bool usable(uint32_t j) const { return valid[j] != 0; }
    nw::Box box(uint32_t j) const { return boxes[j]; }
};

// the directory of `boxes` over a gx x gy grid on their extent (an axis of zero extent: inv = 0)
nw::Grid build(HostDir& d, int gx, int gy) {
    double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    for (const nw::Box& b : d.boxes)
        if (nw::box_ok(b)) x0 = fmin(x0, b.x0), y0 = fmin(y0, b.y0), x1 = fmax(x1, b.x1), y1 = fmax(y1, b.y1);
    const double inv_w = x1 > x0 ? gx / (x1 - x0) : 0.0, inv_h = y1 > y0 ? gy / (y1 - y0) : 0.0;
    const nw::Grid g = nw::make_grid(x0, y0, inv_w, inv_h, gx, gy);
    std::vector<std::vector<int>> cells((size_t)gx * gy);
    for (size_t j = 0; j < d.boxes.size(); ++j) {
        const nw::Box& b = d.boxes[j];
        if (!nw::box_ok(b)) continue;  // (a row without a coordinate has no leaf)
        const int cx0 = nw::cell_of(b.x0, x0, inv_w, gx), cx1 = nw::cell_of(b.x1, x0, inv_w, gx);
        const int cy0 = nw::cell_of(b.y0, y0, inv_h, gy), cy1 = nw::cell_of(b.y1, y0, inv_h, gy);
        for (int cy = cy0; cy <= cy1; ++cy)
            for (int cx = cx0; cx <= cx1; ++cx) cells[(size_t)cy * gx + cx].push_back((int)j);
    }
    d.cell_off.assign(1, 0);
    d.items.clear();
    for (const auto& c : cells) {
        d.items.insert(d.items.end(), c.begin(), c.end());
        d.cell_off.push_back((int)d.items.size());
    }
    return g;
}

uint32_t brute(const nw::Grid& g, const HostDir& d, const nw::Box& L, double max_d, double* bd_out) {
    *bd_out = INFINITY;
    if (!nw::box_ok(L)) return nw::NO_SEED;
    const double m = nw::margin(g, L);
    uint32_t seed = nw::NO_SEED;
    for (uint32_t j = 0; j < d.boxes.size(); ++j) {
        if (!d.valid[j] || !nw::box_ok(d.boxes[j])) continue;
        const double bd = nw::box_distance(L, d.boxes[j]);
        if (!(bd - m <= max_d)) continue;
        if (bd < *bd_out) *bd_out = bd, seed = j;  // (ascending j: the lowest id among equals stays)
    }
    return seed;
}

nw::Box small_box(Rng& r, double lo, double hi, double size) {
    const double x = r.eighth(lo, hi), y = r.eighth(lo, hi);
    return nw::Box{x, y, x + r.eighth(0.0, size), y + r.eighth(0.0, size)};
}

int run_case(const char* name, HostDir& d, int gx, int gy, const std::vector<nw::Box>& lefts) {
    const nw::Grid g = build(d, gx, gy);
    int seeded = 0, bad = 0;
    const double bounds[4] = {INFINITY, 0.0, 6.0, 40.0};
    for (size_t i = 0; i < lefts.size(); ++i) {
        const double max_d = bounds[i & 3];
        double bd_walk, bd_brute;
        const uint32_t s = nw::seed_walk(g, d, lefts[i], max_d, &bd_walk), b = brute(g, d, lefts[i], max_d, &bd_brute);
        seeded += s != nw::NO_SEED;
        if (s != b || memcmp(&bd_walk, &bd_brute, sizeof(double)) != 0) {
            if (++bad <= 5)
                fprintf(stderr, "%s: left %zu (%g %g %g %g) max_d %g: walk %u at %.17g, brute force %u at %.17g\n", name, i, lefts[i].x0, lefts[i].y0,
                        lefts[i].x1, lefts[i].y1, max_d, s, bd_walk, b, bd_brute);
        }
    }
    printf("%s %zu %d %d\n", name, lefts.size(), seeded, bad);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    Rng r{20240607};
    const int N_LEFT = 320;
    auto rights = [&](int n, double size) {
        HostDir d;
        for (int j = 0; j < n; ++j) {
            d.boxes.push_back(small_box(r, 0.0, 100.0, size));
            d.valid.push_back(j % 11 != 5);  // some null rows
            if (j % 13 == 7) d.boxes.back() = nw::Box{NAN, NAN, NAN, NAN};  // some rows without a coordinate
        }
        return d;
    };
    auto lefts_inside = [&](double size) {
        std::vector<nw::Box> v;
        for (int i = 0; i < N_LEFT; ++i) v.push_back(small_box(r, 0.0, 100.0, size));
        v[3] = nw::Box{NAN, 1.0, 2.0, 3.0};  // a left row without a usable box
        return v;
    };
    {  // one cell
        HostDir d = rights(40, 4.0);
        bad += run_case("grid_1x1", d, 1, 1, lefts_inside(3.0));
    }
    {  // 7 x 5
        HostDir d = rights(90, 4.0);
        bad += run_case("grid_7x5", d, 7, 5, lefts_inside(3.0));
    }
    {  // cell borders on the coordinates' lattice: the extent is pinned to [0, 112] x [0, 80] (cells of 16 x 16) and every coordinate is a
       // multiple of 4, so boxes begin exactly on cell borders and an unvisited part is often exactly as far as the best box
        HostDir d;
        d.boxes.push_back(nw::Box{112.0, 80.0, 112.0, 80.0});  // (the far corner first: the nearer rows have higher ids)
        d.valid.push_back(1);
        for (int j = 0; j < 70; ++j) {
            const double x = 4.0 * (double)(r.next() % 28), y = 4.0 * (double)(r.next() % 20);
            d.boxes.push_back(nw::Box{x, y, x + 4.0 * (double)(r.next() % 2), y + 4.0 * (double)(r.next() % 2)});
            d.valid.push_back(1);
        }
        d.boxes.push_back(nw::Box{0.0, 0.0, 0.0, 0.0});
        d.valid.push_back(1);
        std::vector<nw::Box> v;
        for (int i = 0; i < N_LEFT; ++i) {
            const double x = 4.0 * (double)(r.next() % 28), y = 4.0 * (double)(r.next() % 20);
            v.push_back(nw::Box{x, y, x + 4.0 * (double)(r.next() % 2), y + 4.0 * (double)(r.next() % 2)});
        }
        bad += run_case("lattice_borders", d, 7, 5, v);
    }
    {  // every right box on the vertical line x = 3: the x axis has zero extent
        HostDir d = rights(60, 4.0);
        for (nw::Box& b : d.boxes)
            if (nw::box_ok(b)) b.x0 = b.x1 = 3.0;
        std::vector<nw::Box> v = lefts_inside(3.0);
        for (size_t i = 0; i < v.size(); i += 3) v[i].x0 -= 60.0, v[i].x1 -= 60.0;  // on both sides of the line
        bad += run_case("zero_width_axis", d, 7, 5, v);
        for (nw::Box& b : d.boxes)
            if (nw::box_ok(b)) b.y0 = b.y1 = 8.0;  // and both axes: every right box is the point (3, 8)
        bad += run_case("zero_extent", d, 7, 5, v);
    }
    {  // left boxes outside the extent: beyond each side and each corner, near and far
        HostDir d = rights(90, 4.0);
        std::vector<nw::Box> v;
        const double off[8][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {1, 1}, {-1, 1}, {1, -1}};
        for (int i = 0; i < N_LEFT; ++i) {
            nw::Box b = small_box(r, 0.0, 100.0, 3.0);
            const double far = i % 5 == 0 ? 1e6 : (i % 5 == 1 ? 110.0 : 150.0);
            b.x0 += off[i % 8][0] * far, b.x1 += off[i % 8][0] * far, b.y0 += off[i % 8][1] * far, b.y1 += off[i % 8][1] * far;
            v.push_back(b);
        }
        bad += run_case("left_outside", d, 7, 5, v);
    }
    {  // left boxes that cover the whole extent, and more
        HostDir d = rights(90, 4.0);
        std::vector<nw::Box> v;
        for (int i = 0; i < N_LEFT; ++i) v.push_back(nw::Box{-r.eighth(0.0, 50.0), -r.eighth(0.0, 50.0), 104.0 + r.eighth(0.0, 50.0), 104.0 + r.eighth(0.0, 50.0)});
        bad += run_case("left_covers_extent", d, 7, 5, v);
    }
    {  // left boxes spanning 3 x 2 cells of a 7 x 5 grid over [0, 104]^2 (cells about 14.9 x 20.8)
        HostDir d = rights(90, 4.0);
        std::vector<nw::Box> v;
        for (int i = 0; i < N_LEFT; ++i) {
            const double x = r.eighth(0.0, 60.0), y = r.eighth(0.0, 70.0);
            v.push_back(nw::Box{x, y, x + 32.0, y + 22.0});
        }
        bad += run_case("left_3x2_cells", d, 7, 5, v);
    }
    {  // right boxes spanning many cells, one of them every cell, beside small ones; a sparse side so that walks run long
        HostDir d = rights(24, 2.0);
        for (size_t j = 0; j < d.boxes.size(); j += 4)
            if (nw::box_ok(d.boxes[j])) d.boxes[j].x1 += 45.0, d.boxes[j].y1 += 1.0;
        d.boxes[2] = nw::Box{0.0, 0.0, 150.0, 104.0};
        d.valid[2] = 1;
        std::vector<nw::Box> v = lefts_inside(3.0);
        for (size_t i = 0; i < v.size(); i += 2) v[i].x0 += 160.0, v[i].x1 += 160.0;  // half of them to the right of everything
        bad += run_case("right_spans_cells", d, 16, 12, v);
        d.valid[2] = 0;  // the same without the all-covering row
        bad += run_case("right_spans_cells_sparse", d, 16, 12, v);
    }
    return bad ? 1 : 0;
}
