// Stand-alone host program over csrc/gpk_hausdorff.h, csrc/gpk_frechet.h and csrc/gpk_frac.h.  The per-term and per-cell functions
// (pair_seg_dist2, frac_less, sample_coord, see_min, see_max, pick_max, cost; seg_step, dist2, cell) are the ones the kernels compile.
// The schedules of gpk_hausdorff.hip / gpk_frechet.hip are RESTATED here, not shared: lane l of G takes the samples lane l takes on the
// device, the butterfly, the work-group fold and the wavefront's shift register are arrays.
//   hausdorff_host_driver IN OUT
// IN is a sequence of records { int32 k, int32 frechet, then for both sides int32 sequenced (0: POINT / MULTIPOINT), int32 n_seqs and per
// sequence int32 n_coords and double xy[2 n_coords] }.
// OUT receives per record the doubles { H by 8 lanes, H by 32 lanes, H by the work-group schedule, then (frechet != 0, else NaN) F by
// 8 lanes, F by 32 lanes, F by 64 lanes }.
// Built by tests/test_hausdorff_host.py with the host compiler, once plain and once with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_frechet.h"
#include "gpk_hausdorff.h"

namespace {
using gpk::Frac;
namespace hd = gpk::hd;
namespace fr = gpk::fr;

struct P2 {
    double x, y;
};
// RowSeqs of gpk_pairdist.h on the host: flat coordinates and (sequenced rows) the sequence offsets
struct Row {
    bool sequenced;
    std::vector<int> so;  // n_seqs + 1 offsets
    std::vector<P2> xy;
    int n() const { return (int)xy.size(); }
};

bool read_row(FILE* f, Row& r) {
    int32_t h[2];
    if (fread(h, sizeof h, 1, f) != 1 || h[1] < 0) return false;
    r.sequenced = h[0] != 0;
    r.so.assign(1, 0);
    r.xy.clear();
    for (int s = 0; s < h[1]; ++s) {
        int32_t nc;
        if (fread(&nc, sizeof nc, 1, f) != 1 || nc < 0) return false;
        const size_t at = r.xy.size();
        r.xy.resize(at + (size_t)nc);
        if (nc && fread(r.xy.data() + at, sizeof(P2), (size_t)nc, f) != (size_t)nc) return false;
        r.so.push_back((int)r.xy.size());
    }
    return true;
}

// the segment that starts at coordinate c: (c, c + 1) inside its sequence, else (c, c)
void segment(const Row& w, int c, int& ws, P2& p0, P2& p1) {
    p0 = w.xy[(size_t)c];
    p1 = p0;
    if (!w.sequenced) return;
    while (w.so[(size_t)ws + 1] <= c) ++ws;
    if (c + 1 < w.so[(size_t)ws + 1]) p1 = w.xy[(size_t)c + 1];
}

// the sample of slot (c, j) of L, false when the slot does not exist
bool slot(const Row& l, int64_t c, int j, int kk, P2& p) {
    if (c >= l.n()) return false;
    p = l.xy[(size_t)c];
    if (j == 0) return true;
    int s = 0;
    while (l.so[(size_t)s + 1] <= c) ++s;
    if (c + 1 == l.so[(size_t)s + 1]) return false;
    const P2 q = l.xy[(size_t)c + 1];
    p = P2{hd::sample_coord(p.x, q.x, j, kk), hd::sample_coord(p.y, q.y, j, kk)};
    return true;
}

Frac sample_min(const Row& w, P2 p) {
    Frac mn = hd::no_min();
    int ws = 0;
    for (int i = 0; i < w.n(); ++i) {
        P2 p0, p1;
        segment(w, i, ws, p0, p1);
        hd::see_min(mn, gpk::pair_seg_dist2(p.x, p.y, p0.x, p0.y, p1.x, p1.y));
    }
    return mn;
}

// gmax_frac<G>: the xor butterfly, every lane keeps its own value on ties
void butterfly_max(std::vector<Frac>& v) {
    const int G = (int)v.size();
    for (int o = G / 2; o > 0; o >>= 1) {
        std::vector<Frac> w(v);
        for (int l = 0; l < G; ++l)
            if (gpk::frac_less(v[(size_t)l], w[(size_t)(l ^ o)])) v[(size_t)l] = w[(size_t)(l ^ o)];
    }
}

// directed_group<G>: lane l takes slots l, l + G, ...
Frac directed_group(const Row& l, const Row& w, int k, int G) {
    const int kk = l.sequenced ? k : 1;
    const int64_t slots = (int64_t)l.n() * kk;
    std::vector<Frac> mx((size_t)G, hd::no_max());
    for (int lane = 0; lane < G; ++lane) {
        int64_t c = lane / kk;
        int j = lane % kk;
        for (int64_t u0 = 0; u0 < slots; u0 += G) {
            P2 p;
            if (slot(l, c, j, kk, p)) hd::see_max(mx[(size_t)lane], sample_min(w, p));
            j += G;
            c += j / kk;
            j %= kk;
        }
    }
    butterfly_max(mx);
    return mx[0];
}

// directed_workgroup: thread t takes slots t, t + 256, ...; waves of 64 joined by the butterfly, the four waves folded in order
Frac directed_workgroup(const Row& l, const Row& w, int k) {
    const int kk = l.sequenced ? k : 1;
    const int64_t slots = (int64_t)l.n() * kk;
    std::vector<Frac> mx(256, hd::no_max());
    for (int tid = 0; tid < 256; ++tid)
        for (int64_t u = tid; u < slots; u += 256) {
            P2 p;
            if (slot(l, u / kk, (int)(u % kk), kk, p)) hd::see_max(mx[(size_t)tid], sample_min(w, p));
        }
    Frac best = hd::no_max();
    for (int wave = 0; wave < 4; ++wave) {
        std::vector<Frac> v(mx.begin() + 64 * wave, mx.begin() + 64 * (wave + 1));
        butterfly_max(v);
        if (wave == 0)
            best = v[0];
        else
            hd::see_max(best, v[0]);
    }
    return best;
}

int64_t nonempty(const Row& r) {
    if (!r.sequenced) return r.n();
    int64_t q = 0;
    for (size_t s = 0; s + 1 < r.so.size(); ++s) q += r.so[s + 1] > r.so[s] ? 1 : 0;
    return q;
}

// frechet_table<G> of gpk_frechet.hip with the lanes' registers as arrays
double frechet_table(const std::vector<P2>& xw, const std::vector<P2>& xs, int k, int G) {
    const int64_t R = fr::sample_count((int64_t)xw.size(), k), C = fr::sample_count((int64_t)xs.size(), k);
    std::vector<double> bcol((size_t)R, 0.0);
    double answer = 0.0;
    const size_t g = (size_t)G;
    for (int64_t j0 = 0; j0 < C; j0 += G) {
        const bool first = j0 == 0, last = j0 + G >= C;
        std::vector<double> sx(g, 0.0), sy(g, 0.0), cur(g, INFINITY), diag(g, INFINITY), wx(g, 0.0), wy(g, 0.0);
        for (int lane = 0; lane < G; ++lane) {
            const int64_t j = j0 + lane;
            if (j >= C) continue;
            const int64_t c = j / k;
            const int jj = (int)(j - c * k);
            const P2 p = xs[(size_t)c];
            sx[(size_t)lane] = p.x;
            sy[(size_t)lane] = p.y;
            if (jj > 0) {
                const P2 q = xs[(size_t)c + 1];
                sx[(size_t)lane] = fr::sample_coord(p.x, fr::seg_step(p.x, q.x, k), jj);
                sy[(size_t)lane] = fr::sample_coord(p.y, fr::seg_step(p.y, q.y, k), jj);
            }
        }
        if (first) diag[0] = 0.0;
        int64_t wc = 0;
        int wj = 0;
        P2 wp = xw[0], wq = wp;
        double stx = 0.0, sty = 0.0;
        for (int64_t t = 0; t < R + G - 1; ++t) {
            double nx = 0.0, ny = 0.0;
            if (t < R) {
                if (wj == 0 && t + 1 < R) {
                    wq = xw[(size_t)wc + 1];
                    if (k > 1) {
                        stx = fr::seg_step(wp.x, wq.x, k);
                        sty = fr::seg_step(wp.y, wq.y, k);
                    }
                }
                nx = wj == 0 ? wp.x : fr::sample_coord(wp.x, stx, wj);
                ny = wj == 0 ? wp.y : fr::sample_coord(wp.y, sty, wj);
                if (++wj == k) {
                    wj = 0;
                    ++wc;
                    wp = wq;
                }
            }
            const std::vector<double> ox(wx), oy(wy), oc(cur);  // what __shfl_up reads: the values before this step
            for (int lane = 0; lane < G; ++lane) {
                const size_t l = (size_t)lane;
                wx[l] = lane == 0 ? nx : ox[l - 1];
                wy[l] = lane == 0 ? ny : oy[l - 1];
                const int64_t i = t - lane, j = j0 + lane;
                double left = lane == 0 ? ((!first && i < R) ? bcol[(size_t)i] : INFINITY) : oc[l - 1];
                if (j < C && i >= 0 && i < R) {
                    cur[l] = fr::cell(fr::dist2(wx[l], wy[l], sx[l], sy[l]), cur[l], left, diag[l]);
                    if (lane == G - 1 && !last) bcol[(size_t)i] = cur[l];
                    if (i == R - 1 && j == C - 1) answer = cur[l];
                }
                diag[l] = left;
            }
        }
    }
    return answer;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t head[2];
    std::vector<double> out;
    while (fread(head, sizeof head, 1, fi) == 1) {
        const int k = head[0];
        if (k < 1 || k > hd::MAX_SUBDIVISIONS) return 4;
        Row a, b;
        if (!read_row(fi, a) || !read_row(fi, b)) return 3;
        double h[3] = {NAN, NAN, NAN}, f[3] = {NAN, NAN, NAN};
        if (a.n() > 0 && b.n() > 0) {
            const int groups[2] = {8, 32};
            for (int v = 0; v < 2; ++v) h[v] = hd::result(hd::pick_max(directed_group(a, b, k, groups[v]), directed_group(b, a, k, groups[v])));
            h[2] = hd::result(hd::pick_max(directed_workgroup(a, b, k), directed_workgroup(b, a, k)));
            // the cost rule must agree with itself whichever side is called A
            const int64_t sa = hd::sample_count(a.n(), nonempty(a), k, a.sequenced), sb = hd::sample_count(b.n(), nonempty(b), k, b.sequenced);
            if (hd::cost(sa, a.n(), sb, b.n()) != hd::cost(sb, b.n(), sa, a.n())) return 5;
            if (head[1]) {
                const bool a_walks = fr::sample_count(a.n(), k) <= fr::sample_count(b.n(), k);
                const std::vector<P2>&w = a_walks ? a.xy : b.xy, &s = a_walks ? b.xy : a.xy;
                const int lanes[3] = {8, 32, 64};
                for (int v = 0; v < 3; ++v) f[v] = fr::result(frechet_table(w, s, k, lanes[v]));
            }
        }
        out.insert(out.end(), h, h + 3);
        out.insert(out.end(), f, f + 3);
    }
    if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 6;
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 6;
}
