// seqedit_host_driver.cpp — segmentize, remove_repeated_points, reverse and orient_polygons on the CPU: the host-callable routines of
// csrc/gpk_seqedit.h (piece count, interpolation, keep test, the sources of a strip and their bisection, the reversed source, the
// per-lane argmin, its pair reduction, the neighbours of the turn) run as plain loops, strip by strip and lane by lane, the way the
// kernels of csrc/gpk_seqedit.hip run them — every staged window in a buffer of exactly its size, so that a sanitizer sees a read
// past it.  A stand-alone program: tests/test_seqedit_host.py builds it plain and with -fsanitize=address,undefined.
//
//   seqedit_host_driver IN OUT
// IN : i32 op (0 segmentize, 1 remove_repeated_points, 2 reverse, 3 orient), i32 n_levels (1 .. 3), i64 n_rows, f64 m, i32 has_per_row,
//      i32 exterior_cw, i32 group (lanes a ring of the argmin: a power of two), i32 pad; per level: i64 len, i32[len]; i64 n_coords,
//      16 bytes each; f64 per_row[n_rows] when has_per_row
// OUT: i32 status (0, or 1: the result exceeds i32 offsets — nothing follows); i64 len, i32[len]: the innermost offsets; i64 n_coords,
//      16 bytes each; orient: i64 n_rings, u8 reversed[n_rings]
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpk_seqedit.h"

using namespace gpk;

static void die(const char* what) {
    fprintf(stderr, "seqedit_host_driver: %s\n", what);
    exit(2);
}
template <typename T>
static void get(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) die("short read");
}
template <typename T>
static void put(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) die("short write");
}

// the exact sign of orient(a, b, c): the six error-free products summed as an expansion (what gpk_device.h does on the device)
static void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bv = s - a, av = s - bv;
    e = (a - av) + (b - bv);
}
static int exact_orient(se::XY a, se::XY b, se::XY c) {
    const double f[6][2] = {{a.x, b.y}, {-a.x, c.y}, {-c.x, b.y}, {-a.y, b.x}, {a.y, c.x}, {c.y, b.x}};
    double e[12];
    int n = 0;
    for (int i = 0; i < 6; ++i) {
        const double p = f[i][0] * f[i][1];
        const double t[2] = {p, std::fma(f[i][0], f[i][1], -p)};
        for (int k = 0; k < 2; ++k) {
            double q = t[k];
            for (int j = 0; j < n; ++j) {
                double s, err;
                two_sum(q, e[j], s, err);
                e[j] = err;
                q = s;
            }
            e[n++] = q;
        }
    }
    int sign = 0;
    for (int i = 0; i < n; ++i) {
        if (e[i] > 0.0) sign = 1;
        if (e[i] < 0.0) sign = -1;
    }
    return sign;
}

struct Column {
    std::vector<std::vector<int32_t>> off;
    std::vector<gt::Bits16> xy;
    int64_t n_rows = 0;
};

// last[c]: the heads pass
static std::vector<uint8_t> heads(const std::vector<int32_t>& off, int64_t n) {
    std::vector<uint8_t> last((size_t)n, 0);
    for (size_t s = 0; s + 1 < off.size(); ++s)
        if (off[s + 1] > off[s]) last[(size_t)off[s + 1] - 1] = 1;
    return last;
}

// segmentize / remove_repeated_points: the counts in strips of se::STRIP input coordinates, the scan, the offsets, the fill
static int counted(int op, const Column& col, double m, const std::vector<double>& per_row, std::vector<int32_t>& new_off, std::vector<gt::Bits16>& out) {
    const std::vector<int32_t>& off = col.off.back();
    const int64_t n = (int64_t)col.xy.size(), n_seq = (int64_t)off.size() - 1;
    const std::vector<uint8_t> last = heads(off, n);
    std::vector<int32_t> rowstart;
    if (!per_row.empty()) {
        rowstart.resize((size_t)col.n_rows + 1);
        for (int64_t r = 0; r <= col.n_rows; ++r) {
            int64_t a = r;
            for (const auto& o : col.off) a = o[(size_t)a];
            rowstart[(size_t)r] = (int32_t)a;
        }
    }
    auto count = [&](int64_t c) -> int64_t {
        if (op == 1) return se::keeps_at(col.xy.data(), last.data(), c) ? 1 : 0;
        double mc = m;
        if (!per_row.empty()) {
            const gt::Rows all{rowstart.data(), nullptr, nullptr, 0, col.n_rows - 1};
            mc = per_row[(size_t)all.find(c)];
        }
        return se::segment_count(col.xy.data(), last.data(), c, n, mc);
    };
    // pass 0: strip totals; the scan; the total
    const int64_t n_strips_in = (n + se::STRIP - 1) / se::STRIP;
    std::vector<uint64_t> strip_tot((size_t)n_strips_in, 0);
    for (int64_t b = 0; b < n_strips_in; ++b)
        for (int t = 0; t < se::LANES; ++t)
            for (int k = 0; k < se::PER_LANE; ++k) {
                const int64_t c = se::lane_element(b * se::STRIP, t, k);
                if (c < n) strip_tot[(size_t)b] += (uint64_t)count(c);
            }
    uint64_t total = 0;
    for (auto& v : strip_tot) {
        const uint64_t x = v;
        v = total;
        total += x;
    }
    if (total > (uint64_t)INT32_MAX) return 1;
    // pass 1: outpos, and the kept coordinates of remove_repeated_points
    std::vector<int32_t> outpos((size_t)n + 1);
    out.assign((size_t)total, gt::Bits16{0, 0});
    for (int64_t b = 0; b < n_strips_in; ++b) {
        uint64_t o = strip_tot[(size_t)b];
        for (int t = 0; t < se::LANES; ++t)  // (the scan: four consecutive coordinates a lane)
            for (int k = 0; k < se::PER_LANE; ++k) {
                const int64_t c = (b * se::LANES + t) * se::PER_LANE + k;
                if (c >= n) continue;
                const uint64_t cnt = (uint64_t)count(c);
                outpos[(size_t)c] = (int32_t)o;
                if (op == 1 && cnt) out[(size_t)o] = col.xy[(size_t)c];
                o += cnt;
            }
    }
    outpos[(size_t)n] = (int32_t)total;
    new_off.resize((size_t)n_seq + 1);
    for (int64_t s = 0; s <= n_seq; ++s) new_off[(size_t)s] = outpos[(size_t)off[(size_t)s]];
    if (op == 1 || total == 0) return 0;
    // the fill, in output order
    const int64_t n_strips = ((int64_t)total + se::STRIP - 1) / se::STRIP;
    std::vector<int32_t> first_src((size_t)n_strips);
    for (int64_t s = 0; s < n_strips; ++s) first_src[(size_t)s] = gt::strip_first_row(outpos.data(), n, s);
    for (int64_t s = 0; s < n_strips; ++s) {
        const int64_t e0 = s * se::STRIP, e_end = e0 + se::STRIP < (int64_t)total ? e0 + se::STRIP : (int64_t)total;
        const int64_t first = first_src[(size_t)s];
        const int64_t lastc = se::strip_last_source(outpos.data(), first_src.data(), s, n_strips, n, e_end);
        const int64_t w = lastc - first + 2;
        if (w > se::SOURCES) die("a strip with more than STRIP + 1 sources");
        std::vector<int32_t> pos((size_t)w);
        std::vector<gt::Bits16> sxy((size_t)w, gt::Bits16{0, 0});
        for (int64_t k = 0; k < w; ++k) {
            pos[(size_t)k] = outpos[(size_t)(first + k)];
            if (first + k < n) sxy[(size_t)k] = col.xy[(size_t)(first + k)];
        }
        const se::Sources src{pos.data(), sxy.data(), first, lastc};
        for (int t = 0; t < se::LANES; ++t)
            for (int k = 0; k < se::PER_LANE; ++k) {
                const int64_t e = se::lane_element(e0, t, k);
                if (e < e_end) out[(size_t)e] = src.value(e);
            }
    }
    return 0;
}

// the per-ring argmin with `group` lanes and the xor-tree of the kernels; every lane must end with the same winner
static se::Cand ring_argmin(const gt::Bits16* xy, int64_t lo, int64_t hi, int group) {
    std::vector<se::Cand> lane((size_t)group);
    for (int l = 0; l < group; ++l) lane[(size_t)l] = se::lane_argmin(xy, lo, hi, l, group);
    for (int o = group / 2; o > 0; o >>= 1) {
        std::vector<se::Cand> next((size_t)group);
        for (int l = 0; l < group; ++l) next[(size_t)l] = se::merge(lane[(size_t)l], lane[(size_t)(l ^ o)]);
        lane = next;
    }
    for (int l = 1; l < group; ++l)
        if (lane[(size_t)l].i != lane[0].i || lane[(size_t)l].bad != lane[0].bad) die("the lanes of a group disagree");
    return lane[0];
}

static void reversed(const Column& col, bool orient, bool exterior_cw, int group, std::vector<gt::Bits16>& out, std::vector<uint8_t>& rev) {
    const std::vector<int32_t>& off = col.off.back();
    const int64_t n = (int64_t)col.xy.size(), n_seq = (int64_t)off.size() - 1;
    if (orient) {
        if (col.off.size() < 2) die("orient: a polygonal column has two levels at least");
        const std::vector<int32_t>& poly = col.off[col.off.size() - 2];
        std::vector<uint8_t> shell((size_t)n_seq, 0);
        for (size_t p = 0; p + 1 < poly.size(); ++p)
            if (poly[p + 1] > poly[p]) shell[(size_t)poly[p]] = 1;
        rev.assign((size_t)n_seq, 0);
        for (int64_t r = 0; r < n_seq; ++r) {
            const int64_t lo = off[(size_t)r], hi = off[(size_t)r + 1];
            const se::Cand best = ring_argmin(col.xy.data(), lo, hi, group);
            int64_t u, v, w;
            if (!se::ring_turn(col.xy.data(), lo, hi, best, &u, &v, &w)) continue;
            const int s = exact_orient(se::as_xy(col.xy[(size_t)u]), se::as_xy(col.xy[(size_t)v]), se::as_xy(col.xy[(size_t)w]));
            rev[(size_t)r] = se::reverses(s, shell[(size_t)r] != 0, exterior_cw) ? 1 : 0;
        }
    }
    out.assign((size_t)n, gt::Bits16{0, 0});
    if (n == 0) return;
    const int64_t n_strips = (n + se::STRIP - 1) / se::STRIP;
    std::vector<int32_t> first_seq((size_t)n_strips);
    for (int64_t s = 0; s < n_strips; ++s) first_seq[(size_t)s] = gt::strip_first_row(off.data(), n_seq, s);
    for (int64_t s = 0; s < n_strips; ++s) {
        const int64_t e0 = s * se::STRIP, e_end = e0 + se::STRIP < n ? e0 + se::STRIP : n;
        gt::Rows rows = gt::strip_rows(off.data(), n_seq, first_seq.data(), s, n_strips);
        const int64_t w = rows.last - rows.first + 1;
        std::vector<int32_t> win;
        if (w <= gt::WINDOW) {
            for (int64_t k = 0; k < w + 1; ++k) win.push_back(off[(size_t)(rows.first + k)]);
            rows.win = win.data();
        }
        for (int t = 0; t < se::LANES; ++t)
            for (int k = 0; k < se::PER_LANE; ++k) {
                const int64_t e = se::lane_element(e0, t, k);
                if (e < e_end) out[(size_t)e] = col.xy[(size_t)se::reverse_source(rows, orient ? rev.data() : nullptr, e)];
            }
    }
}

int main(int argc, char** argv) {
    if (argc != 3) die("usage: seqedit_host_driver IN OUT");
    FILE* f = fopen(argv[1], "rb");
    if (!f) die("cannot open the input");
    int32_t op = 0, n_levels = 0, has_per_row = 0, exterior_cw = 0, group = 1, pad = 0;
    double m = 0;
    Column col;
    get(f, &op, 1);
    get(f, &n_levels, 1);
    get(f, &col.n_rows, 1);
    get(f, &m, 1);
    get(f, &has_per_row, 1);
    get(f, &exterior_cw, 1);
    get(f, &group, 1);
    get(f, &pad, 1);
    if (op < 0 || op > 3 || n_levels < 1 || n_levels > gt::MAX_LEVELS || col.n_rows < 0 || group < 1 || (group & (group - 1))) die("bad header");
    col.off.resize((size_t)n_levels);
    for (auto& o : col.off) {
        int64_t len = 0;
        get(f, &len, 1);
        o.resize((size_t)len);
        get(f, o.data(), o.size());
    }
    int64_t n_coords = 0;
    get(f, &n_coords, 1);
    col.xy.resize((size_t)n_coords);
    get(f, col.xy.data(), col.xy.size());
    std::vector<double> per_row;
    if (has_per_row) {
        per_row.resize((size_t)col.n_rows);
        get(f, per_row.data(), per_row.size());
    }
    fclose(f);

    std::vector<int32_t> new_off = col.off.back();
    std::vector<gt::Bits16> out;
    std::vector<uint8_t> rev;
    int32_t status = 0;
    if (op <= 1) {
        if (n_coords > 0)
            status = counted(op, col, m, per_row, new_off, out);
    } else {
        reversed(col, op == 3, exterior_cw != 0, group, out, rev);
    }

    FILE* g = fopen(argv[2], "wb");
    if (!g) die("cannot open the output");
    put(g, &status, 1);
    if (status == 0) {
        const int64_t len = (int64_t)new_off.size(), n_out = (int64_t)out.size();
        put(g, &len, 1);
        put(g, new_off.data(), new_off.size());
        put(g, &n_out, 1);
        put(g, out.data(), out.size());
        if (op == 3) {
            const int64_t n_rings = (int64_t)rev.size();
            put(g, &n_rings, 1);
            put(g, rev.data(), rev.size());
        }
    }
    fclose(g);
    return 0;
}
