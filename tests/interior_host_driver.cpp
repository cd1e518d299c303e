// Stand-alone host program over the rules of csrc/gpk_interior.h: the very functions the GPU lanes run, applied sequentially on the CPU.
//   interior_host_driver IN OUT
// IN is a sequence of records { int32 kind (the GPK_GEOM_* code), int32 n_parts, then per part int32 n_seqs, then per sequence int32
// n_coords and double xy[2 n_coords] } (a lineal or puntal row: one part; a point: one sequence of one coordinate).
// OUT receives per record the doubles { valid, x, y, width, n_members, then per non-empty member: scanY, number of crossings }.
// Built by tests/test_interior_host.py with the host compiler, once plain and once with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_interior.h"

namespace {
namespace ip = gpk::ip;
struct P2 {
    double x, y;
};
typedef std::vector<P2> Seq;
typedef std::vector<Seq> Part;
typedef std::vector<Part> Geom;

bool read_geom(FILE* f, Geom& g) {
    int32_t np;
    if (fread(&np, sizeof np, 1, f) != 1 || np < 0) return false;
    g.assign((size_t)np, Part());
    for (auto& part : g) {
        int32_t ns;
        if (fread(&ns, sizeof ns, 1, f) != 1 || ns < 0) return false;
        part.assign((size_t)ns, Seq());
        for (auto& seq : part) {
            int32_t nc;
            if (fread(&nc, sizeof nc, 1, f) != 1 || nc < 0) return false;
            seq.resize((size_t)nc);
            if (nc && fread(seq.data(), sizeof(P2), (size_t)nc, f) != (size_t)nc) return false;
        }
    }
    return true;
}

bool finite(const Geom& g) {
    for (const Part& part : g)
        for (const Seq& s : part)
            for (P2 p : s)
                if (!(std::fabs(p.x) < INFINITY) || !(std::fabs(p.y) < INFINITY)) return false;
    return true;
}
size_t coords(const Geom& g) {
    size_t n = 0;
    for (const Part& part : g)
        for (const Seq& s : part) n += s.size();
    return n;
}

struct Crossing {
    double x;
    int e;
};

void polygonal(const Geom& g, std::vector<double>& out) {
    ip::RowPoint pt{NAN, NAN, NAN};
    bool ok = false;
    std::vector<double> members;
    if (coords(g) > 0 && finite(g)) {
        for (const Part& part : g) {
            if (part.empty() || part[0].empty()) continue;
            if (!ok) {
                pt = ip::RowPoint{0.0, part[0][0].x, part[0][0].y};
                ok = true;
            }
            double miny = INFINITY, maxy = -INFINITY;
            for (const Seq& r : part)
                for (P2 p : r) miny = std::fmin(miny, p.y), maxy = std::fmax(maxy, p.y);
            const double centre = ip::centre_y(miny, maxy);
            double lo = miny, hi = maxy;
            for (const Seq& r : part)
                for (P2 p : r) ip::scan_update(p.y, centre, lo, hi);
            const double scan = ip::scan_y(lo, hi);
            std::vector<Crossing> cr;
            int e = 0;
            for (const Seq& r : part) {
                for (size_t i = 0; i + 1 < r.size(); ++i)
                    if (ip::edge_counts(r[i].y, r[i + 1].y, scan)) cr.push_back(Crossing{ip::crossing_x(r[i].x, r[i].y, r[i + 1].x, r[i + 1].y, scan), e + (int)i});
                e += (int)r.size();
            }
            ip::Section best = ip::no_section();
            for (const Crossing& c : cr) {  // the device's ranking: every crossing against all of them
                ip::Ranked rk = ip::ranked_start();
                for (const Crossing& o : cr) ip::ranked_see(rk, c.x, c.e, o.x, o.e);
                if (!(rk.rank & 1) && rk.has_succ) ip::section_propose(best, c.x, rk.succ_x, rk.rank);
            }
            ip::member_fold(pt, best, scan);
            members.push_back(scan);
            members.push_back((double)cr.size());
        }
    }
    out.insert(out.end(), {ok ? 1.0 : 0.0, ok ? pt.x : NAN, ok ? pt.y : NAN, ok ? pt.width : NAN, (double)(members.size() / 2)});
    out.insert(out.end(), members.begin(), members.end());
}

// the length-weighted centroid of the sequences in f64, the mean for points
void vertices(const Geom& g, bool lineal, std::vector<double>& out) {
    const Part empty;
    const Part& seqs = g.empty() ? empty : g[0];
    ip::Nearest inner = ip::no_nearest(), ends = ip::no_nearest();
    std::vector<P2> flat;
    if (coords(g) > 0 && finite(g)) {
        double cx = 0.0, cy = 0.0;
        if (lineal) {
            // members of positive length weigh in by length; when there is none, every member gives its start once per segment (a member
            // of one coordinate: once) — geo's dimension rule, what gpk_centroid returns
            double len = 0.0, mx = 0.0, my = 0.0, k = 0.0, sx = 0.0, sy = 0.0;
            for (const Seq& s : seqs) {
                if (s.empty()) continue;
                const double w = s.size() == 1 ? 1.0 : (double)(s.size() - 1);
                k += w, sx += s[0].x * w, sy += s[0].y * w;
                for (size_t i = 0; i + 1 < s.size(); ++i) {
                    const double dx = s[i + 1].x - s[i].x, dy = s[i + 1].y - s[i].y, l = std::sqrt(dx * dx + dy * dy);
                    len += l;
                    mx += l * ((s[i].x + s[i + 1].x) / 2);
                    my += l * ((s[i].y + s[i + 1].y) / 2);
                }
            }
            cx = len > 0.0 ? mx / len : sx / k;
            cy = len > 0.0 ? my / len : sy / k;
        } else {
            size_t n = 0;
            for (const Seq& s : seqs)
                for (P2 p : s) cx += p.x, cy += p.y, ++n;
            cx /= (double)n;
            cy /= (double)n;
        }
        for (const Seq& s : seqs)
            for (size_t i = 0; i < s.size(); ++i) {
                const bool end = lineal && (i == 0 || i + 1 == s.size());
                ip::nearest_see(end ? ends : inner, ip::dist2(s[i].x, s[i].y, cx, cy), (int)flat.size());
                flat.push_back(s[i]);
            }
    }
    const ip::Nearest n = inner.index != ip::NO_RANK ? inner : ends;
    const bool ok = n.index != ip::NO_RANK;
    out.insert(out.end(), {ok ? 1.0 : 0.0, ok ? flat[(size_t)n.index].x : NAN, ok ? flat[(size_t)n.index].y : NAN, NAN, 0.0});
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t kind;
    std::vector<double> out;
    while (fread(&kind, sizeof kind, 1, fi) == 1) {
        Geom g;
        if (!read_geom(fi, g)) return 3;
        if (kind == 3 || kind == 6)
            polygonal(g, out);
        else
            vertices(g, kind == 1 || kind == 5, out);
    }
    if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 6;
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 6;
}
