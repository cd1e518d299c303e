// The k-seed walk of gpk_knn_join (geopolars_amd/csrc/gpk_knnwalk.h) on the CPU: a stand-alone program, no GPU.  For every case it builds
// a bbox grid directory on the host with the header's own cell function (a right row is listed in every cell its closed box meets, ids
// ascending within a cell — the shape of the library's directory), runs the walk for a few hundred left boxes with K cycling through
// 1, 2, 5, 9, 33 and 65 and max_d through INFINITY, 6, 40 and 150, and compares its slots with brute force: the K lowest (far distance,
// row) keys among the usable right rows with far distance <= max_d, each row once, ascending — same rows, same distance bits, same
// count.  Coordinates are multiples of 1/8, so equal far distances (ties) are common.
// Output: one line per case, "<name> <left boxes> <full lists> <short lists> <mismatches>"; exit status 1 when a case has a mismatch.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "gpk_knnwalk.h"

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
    double eighth(double lo, double hi) {  // a multiple of 1/8 in [lo, hi]
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

// exactly K slots: the sanitized build catches a walk that touches slot K
struct HostSlots {
    std::vector<double> f;
    std::vector<uint32_t> r;
    explicit HostSlots(int K) : f((size_t)K, -1.0), r((size_t)K, 0xDEADBEEFu) {}
    double& far(int s) { return f.at((size_t)s); }
    uint32_t& row(int s) { return r.at((size_t)s); }
};

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

std::vector<std::pair<double, uint32_t>> brute(const HostDir& d, const nw::Box& L, double max_d, int K) {
    std::vector<std::pair<double, uint32_t>> keys;
    if (!nw::box_ok(L)) return keys;
    for (uint32_t j = 0; j < d.boxes.size(); ++j) {
        if (!d.valid[j] || !nw::box_ok(d.boxes[j])) continue;
        const double fd = nw::box_far_distance(L, d.boxes[j]);
        if (fd <= max_d) keys.emplace_back(fd, j);
    }
    std::sort(keys.begin(), keys.end());
    if ((int)keys.size() > K) keys.resize((size_t)K);
    return keys;
}

nw::Box small_box(Rng& r, double lo, double hi, double size) {
    const double x = r.eighth(lo, hi), y = r.eighth(lo, hi);
    return nw::Box{x, y, x + r.eighth(0.0, size), y + r.eighth(0.0, size)};
}

int run_case(const char* name, HostDir& d, int gx, int gy, const std::vector<nw::Box>& lefts) {
    const nw::Grid g = build(d, gx, gy);
    int full = 0, fewer = 0, bad = 0;
    const double bounds[4] = {INFINITY, 6.0, 40.0, 150.0};
    const int ks[6] = {1, 2, 5, 9, 33, 65};
    for (size_t i = 0; i < lefts.size(); ++i) {
        const double max_d = bounds[i & 3];
        const int K = ks[(i / 4) % 6];
        HostSlots slots(K);
        const int held = nw::knn_seed_walk(g, d, lefts[i], max_d, K, slots);
        const auto want = brute(d, lefts[i], max_d, K);
        bool ok = held == (int)want.size();
        for (int s = 0; ok && s < held; ++s) ok = slots.row(s) == want[(size_t)s].second && memcmp(&slots.far(s), &want[(size_t)s].first, sizeof(double)) == 0;
        full += held == K;
        fewer += held < K;
        if (!ok && ++bad <= 5)
            fprintf(stderr, "%s: left %zu (%g %g %g %g) max_d %g K %d: walk holds %d, brute force %zu\n", name, i, lefts[i].x0, lefts[i].y0, lefts[i].x1,
                    lefts[i].y1, max_d, K, held, want.size());
    }
    printf("%s %zu %d %d %d\n", name, lefts.size(), full, fewer, bad);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    Rng r{20240911};
    const int N_LEFT = 360;
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
    {  // random grids
        HostDir d = rights(300, 4.0);
        bad += run_case("grid_7x5", d, 7, 5, lefts_inside(3.0));
        bad += run_case("grid_23x19", d, 23, 19, lefts_inside(3.0));
    }
    {  // points on an integer lattice: far distance == distance, whole rings of ties, cell borders on the coordinates
        HostDir d;
        for (int y = 0; y <= 16; ++y)
            for (int x = 0; x <= 16; ++x) {
                d.boxes.push_back(nw::Box{4.0 * x, 4.0 * y, 4.0 * x, 4.0 * y});
                d.valid.push_back(1);
            }
        std::vector<nw::Box> v;
        for (int i = 0; i < N_LEFT; ++i) {
            const double x = 4.0 * (double)(r.next() % 17), y = 4.0 * (double)(r.next() % 17);
            v.push_back(nw::Box{x, y, x, y});
        }
        bad += run_case("lattice_points", d, 8, 8, v);
    }
    {  // long diagonal boxes listed in many cells beside short ones
        HostDir d = rights(200, 2.0);
        for (size_t j = 0; j < 40; ++j) {
            const double o = r.eighth(0.0, 20.0);
            d.boxes[j * 5] = nw::Box{o, o, 80.0 + o, 80.0 + o};
        }
        bad += run_case("long_boxes", d, 16, 12, lefts_inside(1.0));
    }
    {  // every right box on the vertical line x = 3: the x axis has zero extent; then both axes
        HostDir d = rights(120, 4.0);
        for (nw::Box& b : d.boxes)
            if (nw::box_ok(b)) b.x0 = b.x1 = 3.0;
        std::vector<nw::Box> v = lefts_inside(3.0);
        for (size_t i = 0; i < v.size(); i += 3) v[i].x0 -= 60.0, v[i].x1 -= 60.0;
        bad += run_case("zero_width_axis", d, 7, 5, v);
        for (nw::Box& b : d.boxes)
            if (nw::box_ok(b)) b.y0 = b.y1 = 8.0;
        bad += run_case("zero_extent", d, 7, 5, v);
    }
    {  // left boxes outside the extent: beyond each side and each corner, near and far
        HostDir d = rights(150, 4.0);
        std::vector<nw::Box> v;
        const double off[8][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {1, 1}, {-1, 1}, {1, -1}};
        for (int i = 0; i < N_LEFT; ++i) {
            nw::Box b = small_box(r, 0.0, 100.0, 3.0);
            const double far = i % 5 == 0 ? 1e6 : (i % 5 == 1 ? 110.0 : 30.0);
            b.x0 += off[i % 8][0] * far, b.x1 += off[i % 8][0] * far, b.y0 += off[i % 8][1] * far, b.y1 += off[i % 8][1] * far;
            v.push_back(b);
        }
        bad += run_case("left_outside", d, 7, 5, v);
    }
    {  // left boxes that cover the whole extent, and left boxes spanning several cells
        HostDir d = rights(150, 4.0);
        std::vector<nw::Box> v;
        for (int i = 0; i < N_LEFT; ++i) {
            if (i & 1) {
                v.push_back(nw::Box{-r.eighth(0.0, 50.0), -r.eighth(0.0, 50.0), 104.0 + r.eighth(0.0, 50.0), 104.0 + r.eighth(0.0, 50.0)});
            } else {
                const double x = r.eighth(0.0, 60.0), y = r.eighth(0.0, 70.0);
                v.push_back(nw::Box{x, y, x + 32.0, y + 22.0});
            }
        }
        bad += run_case("left_spans_cells", d, 7, 5, v);
    }
    {  // fewer usable right rows than K
        HostDir d = rights(12, 4.0);
        bad += run_case("few_rights", d, 4, 4, lefts_inside(3.0));
    }
    return bad ? 1 : 0;
}
