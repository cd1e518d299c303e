// Stand-alone host program over the pair terms of csrc/gpk_overlay.h: the very functions the GPU lanes run, summed sequentially on the
// CPU with an exact __int128 orientation (the fixture's coordinates are integers, at either placement).
//   overlay_host_driver IN OUT
// IN is a sequence of records { int32 what (0 area, 1 length), geometry A, geometry B }, a geometry being { int32 n_parts, then per
// part int32 n_rings, then per ring int32 n_coords and double xy[2 n_coords] } (a line: one part whose rings are its sequences).
// OUT receives one double per record.  Built by tests/test_overlay_host.py with the host compiler, once plain and once with
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_overlay.h"

namespace {
using gpk::ov::P2;
typedef std::vector<P2> Seq;
typedef std::vector<Seq> Part;
typedef std::vector<Part> Geom;
struct Edge {
    P2 a, b;
};
struct Box {
    double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    void add(P2 p) {
        x0 = fmin(x0, p.x), y0 = fmin(y0, p.y), x1 = fmax(x1, p.x), y1 = fmax(y1, p.y);
    }
    bool misses(P2 a, P2 b) const { return fmax(a.x, b.x) < x0 || fmin(a.x, b.x) > x1 || fmax(a.y, b.y) < y0 || fmin(a.y, b.y) > y1; }
};

struct ExactOrient {
    int operator()(P2 a, P2 b, P2 c) const {
        const __int128 ax = (int64_t)a.x, ay = (int64_t)a.y, bx = (int64_t)b.x, by = (int64_t)b.y, cx = (int64_t)c.x, cy = (int64_t)c.y;
        const __int128 d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
        return d > 0 ? 1 : (d < 0 ? -1 : 0);
    }
};

bool read_geom(FILE* f, Geom& g) {
    int32_t np;
    if (fread(&np, sizeof np, 1, f) != 1 || np < 0) return false;
    g.assign((size_t)np, Part());
    for (auto& part : g) {
        int32_t nr;
        if (fread(&nr, sizeof nr, 1, f) != 1 || nr < 0) return false;
        part.assign((size_t)nr, Seq());
        for (auto& ring : part) {
            int32_t nc;
            if (fread(&nc, sizeof nc, 1, f) != 1 || nc < 0) return false;
            ring.resize((size_t)nc);
            if (nc && fread(ring.data(), sizeof(P2), (size_t)nc, f) != (size_t)nc) return false;
        }
    }
    return true;
}

// the edges of a polygonal geometry with its interior on their left, and the box of its shells
void oriented_edges(const Geom& g, std::vector<Edge>& out, Box& box) {
    for (const Part& part : g) {
        if (part.empty() || part[0].empty()) continue;
        for (P2 p : part[0]) box.add(p);
        for (size_t r = 0; r < part.size(); ++r) {
            const Seq& v = part[r];
            if (v.size() < 2) continue;
            __int128 twice = 0;  // the shoelace sum, exact
            for (size_t i = 0; i + 1 < v.size(); ++i)
                twice += (__int128)(int64_t)v[i].x * (int64_t)v[i + 1].y - (__int128)(int64_t)v[i + 1].x * (int64_t)v[i].y;
            const bool keep = (twice > 0) != (r > 0);
            for (size_t i = 0; i + 1 < v.size(); ++i) {
                const P2 a = v[keep ? i : i + 1], b = v[keep ? i + 1 : i];
                if (a.x != b.x || a.y != b.y) out.push_back(Edge{a, b});
            }
        }
    }
}

double green_sum(const std::vector<Edge>& X, const std::vector<Edge>& Y, const Box& box_y, P2 o, bool x_is_a) {
    double acc = 0.0;
    for (const Edge& e : X) {
        if (box_y.misses(e.a, e.b)) continue;
        double tau = 0.0;
        for (const Edge& f : Y) tau += gpk::ov::inside_term(e.a, e.b, f.a, f.b, x_is_a, ExactOrient{});
        acc += gpk::ov::cross_at(e.a, e.b, o) * tau;
    }
    return acc;
}

double area(const Geom& A, const Geom& B) {
    std::vector<Edge> ea, eb;
    Box ba, bb;
    oriented_edges(A, ea, ba);
    oriented_edges(B, eb, bb);
    if (ea.empty() || eb.empty()) return NAN;
    if (ba.x1 < bb.x0 || ba.x0 > bb.x1 || ba.y1 < bb.y0 || ba.y0 > bb.y1) return 0.0;
    const P2 o = gpk::ov::local_origin(ba.x0, ba.y0, ba.x1, ba.y1, bb.x0, bb.y0, bb.x1, bb.y1);
    return fmax(0.0, 0.5 * (green_sum(ea, eb, bb, o, true) + green_sum(eb, ea, ba, o, false)));
}

double length(const Geom& L, const Geom& Q) {
    std::vector<Edge> eq;
    Box bq, bl;
    oriented_edges(Q, eq, bq);
    size_t coords = 0;
    for (const Part& part : L)
        for (const Seq& s : part)
            for (P2 p : s) bl.add(p), ++coords;
    if (eq.empty() || coords == 0) return NAN;
    if (bl.x1 < bq.x0 || bl.x0 > bq.x1 || bl.y1 < bq.y0 || bl.y0 > bq.y1) return 0.0;
    double acc = 0.0;
    for (const Part& part : L)
        for (const Seq& s : part)
            for (size_t i = 0; i + 1 < s.size(); ++i) {
                const P2 p = s[i], q = s[i + 1];
                if ((p.x == q.x && p.y == q.y) || bq.misses(p, q)) continue;
                double t = 0.0;
                for (const Edge& f : eq)
                    t += gpk::ov::inside_term(p, q, f.a, f.b, true, ExactOrient{}) + gpk::ov::along_term(p, q, f.a, f.b, ExactOrient{});
                const double dx = q.x - p.x, dy = q.y - p.y;
                acc += sqrt(dx * dx + dy * dy) * t;
            }
    return fmax(0.0, acc);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t what;
    while (fread(&what, sizeof what, 1, fi) == 1) {
        Geom A, B;
        if (!read_geom(fi, A) || !read_geom(fi, B)) return 3;
        const double m = what == 0 ? area(A, B) : length(A, B);
        fwrite(&m, sizeof m, 1, fo);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 6;
}
