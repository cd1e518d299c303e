// Stand-alone host program over the rules of csrc/gpk_minbound.h: the very functions the GPU lanes run, applied sequentially on the CPU.
//   minbound_host_driver IN OUT
// IN is a sequence of records { int32 n_coords (-1: a null row), double xy[2 n_coords] (the row's coordinates: tested for finiteness),
// int32 h, double hull[2 h] (the row's hull ring as gpk_convex_hull writes it, closing vertex dropped; h = 0 when the row has no
// coordinate or a non-finite one) }.
// OUT receives per record 27 doubles { valid, the ring c0 c1 c2 c3 c0 (10), centre x, centre y, radius, circle iterations, chosen edge,
// the ring of the full scan over every edge and vertex (10), the size of the circle's support }.  The ring is the answer as the device
// computes it: the full scan up to MBG_SMALL_HULL hull vertices, above that the rotating calipers in the work-group's chunks (one chunk
// of ceil(h / MBG_BIG_THREADS) edges a thread, each started afresh).
// Built by tests/test_minbound_host.py with the host compiler, once plain and once with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_minbound.h"

namespace {
namespace mb = gpk::mb;
struct P2 {
    double x, y;
};

bool read_points(FILE* f, int32_t n, std::vector<P2>& p) {
    p.resize((size_t)n);
    return n == 0 || fread(p.data(), sizeof(P2), (size_t)n, f) == (size_t)n;
}

void row(const std::vector<P2>& xy, bool null_row, const std::vector<P2>& v, std::vector<double>& out) {
    bool ok = !null_row && !xy.empty() && !v.empty();
    for (P2 p : xy) ok = ok && std::fabs(p.x) < INFINITY && std::fabs(p.y) < INFINITY;
    if (!ok) {
        out.push_back(0.0);
        out.insert(out.end(), 26, NAN);
        return;
    }
    const int h = (int)v.size();
    mb::Rect r, scan;
    double cx, cy, rad, iters = 0.0, edge = -1.0, ns = 2.0;
    if (h <= 2) {
        const P2 p = v[0], q = v[(size_t)h - 1];
        r = scan = mb::rect_flat(p.x, p.y, q.x, q.y);
        const mb::Circle k = mb::circle_start(q.x - p.x, q.y - p.y, 1);
        cx = p.x + k.cx, cy = p.y + k.cy, rad = std::sqrt(k.r2);
    } else {
        mb::Edge best = mb::no_edge();
        for (int i = 0; i < h; ++i) {
            const P2 p = v[(size_t)i], q = v[(size_t)(i + 1 == h ? 0 : i + 1)];
            const double dx = q.x - p.x, dy = q.y - p.y;
            mb::Extent e = mb::extent_start();
            for (P2 w : v) mb::extent_see(e, p.x, p.y, dx, dy, w.x, w.y);
            const mb::Edge cand = mb::edge_of(i, dx, dy, e);
            if (mb::edge_better(cand, best)) best = cand;
        }
        auto rect_on = [&](const mb::Edge& e) {
            const P2 p = v[(size_t)e.i], q = v[(size_t)(e.i + 1 == h ? 0 : e.i + 1)];
            return mb::rect_corners(p.x, p.y, q.x - p.x, q.y - p.y, e);
        };
        scan = rect_on(best);
        if (h > mb::MBG_SMALL_HULL) {  // the work-group's schedule
            const int per = (h + mb::MBG_BIG_THREADS - 1) / mb::MBG_BIG_THREADS;
            best = mb::no_edge();
            for (int e0 = 0; e0 < h; e0 += per) {
                mb::Calipers cal{0, 0, 0};
                for (int i = e0; i < e0 + per && i < h; ++i) {
                    const mb::Edge cand = mb::caliper_edge([&](int k) { return v[(size_t)k]; }, h, i, i == e0, cal);
                    if (mb::edge_better(cand, best)) best = cand;
                }
            }
        }
        r = rect_on(best);
        edge = (double)best.i;
        const P2 v0 = v[0];
        auto farthest = [&](double ox, double oy) {
            mb::Far f = mb::no_far();
            for (int k = 0; k < h; ++k) mb::far_see(f, mb::dist2(v[(size_t)k].x - v0.x, v[(size_t)k].y - v0.y, ox, oy), k);
            return f;
        };
        mb::Far f = farthest(0.0, 0.0);
        mb::Circle cir = mb::circle_start(v[(size_t)f.index].x - v0.x, v[(size_t)f.index].y - v0.y, f.index);
        bool done = false;
        int it = 0;
        for (; it < MBG_CIRCLE_ITERS; ++it) {
            f = farthest(cir.cx, cir.cy);
            if (mb::circle_done(cir, f)) {
                done = true;
                break;
            }
            cir = mb::circle_step(cir, v[(size_t)f.index].x - v0.x, v[(size_t)f.index].y - v0.y, f.index);
        }
        if (!done) cir.r2 = farthest(cir.cx, cir.cy).d2;
        iters = (double)it;
        cx = v0.x + cir.cx, cy = v0.y + cir.cy, rad = std::sqrt(cir.r2);
        ns = (double)cir.ns;
    }
    out.insert(out.end(), {1.0, r.x0, r.y0, r.x1, r.y1, r.x2, r.y2, r.x3, r.y3, r.x0, r.y0, cx, cy, rad, iters, edge,
                           scan.x0, scan.y0, scan.x1, scan.y1, scan.x2, scan.y2, scan.x3, scan.y3, scan.x0, scan.y0, ns});
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t n;
    std::vector<double> out;
    std::vector<P2> xy, hull;
    while (fread(&n, sizeof n, 1, fi) == 1) {
        int32_t h;
        if (n < -1 || !read_points(fi, n < 0 ? 0 : n, xy)) return 3;
        if (fread(&h, sizeof h, 1, fi) != 1 || h < 0 || !read_points(fi, h, hull)) return 3;
        row(xy, n < 0, hull, out);
    }
    if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 6;
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 6;
}
