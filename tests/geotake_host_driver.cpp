// geotake_host_driver.cpp — the gather of geometry rows on the CPU: the host-callable routines of csrc/gpk_geotake.h (row_ranges, the
// strip's rows, the window, the locate step, the two payloads) run as plain loops, strip by strip and lane by lane, the way
// geotake_fill_kernel runs them — the window staged in a buffer of exactly its size (so a sanitizer sees a read past it) when it has at
// most gt::WINDOW rows, bisected in the row starts themselves otherwise.  A stand-alone program: tests/test_geotake_host.py builds it
// plain and with -fsanitize=address,undefined.
//
//   geotake_host_driver IN OUT
// IN : i32 n_levels, i64 n_rows, i64 n_idx; per level: i64 len, i32[len]; i64 n_coords, 16 bytes each; i64 idx[n_idx]
// OUT: per level: i64 len, i32[len]; i64 n_coords, 16 bytes each; u8 in_range[n_idx]
// (n_levels == 0: a POINT column — out[i] = src[idx[i]], (NaN, NaN) for an index outside [0, n_rows))
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpk_geotake.h"

using namespace gpk;

static void die(const char* what) {
    fprintf(stderr, "geotake_host_driver: %s\n", what);
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

// every strip of a level, every lane of the strip
template <class Payload>
static void fill(const Payload& p, const std::vector<int32_t>& start, int64_t n_slots, int64_t total) {
    const int64_t n_strips = (total + gt::STRIP - 1) / gt::STRIP;
    std::vector<int32_t> first_row((size_t)n_strips);  // the level's strip table
    for (int64_t s = 0; s < n_strips; ++s) first_row[s] = gt::strip_first_row(start.data(), n_slots, s);
    for (int64_t s = 0; s < n_strips; ++s) {
        const int64_t e0 = s * gt::STRIP, e_end = e0 + gt::STRIP < total ? e0 + gt::STRIP : total;
        gt::Rows rows = gt::strip_rows(start.data(), n_slots, first_row.data(), s, n_strips);
        const int64_t w = rows.last - rows.first + 1;
        std::vector<int32_t> win, shift_win;
        if (w <= gt::WINDOW) {
            for (int64_t k = 0; k < w; ++k) {
                win.push_back(start[rows.first + k]);
                shift_win.push_back(p.src_lo[rows.first + k] - start[rows.first + k]);
            }
            rows.win = win.data();
            rows.shift_win = shift_win.data();
        }
        for (int t = 0; t < gt::LANES; ++t) {
            typename Payload::T v[gt::PER_LANE];
            const unsigned have = gt::lane_values(p, rows, e0, e_end, t, v);
            for (int k = 0; k < gt::PER_LANE; ++k)
                if (have & (1u << k)) p.dst[gt::lane_element<Payload>(e0, t, k)] = v[k];
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 3) die("usage: geotake_host_driver IN OUT");
    FILE* f = fopen(argv[1], "rb");
    if (!f) die("cannot open the input");
    int32_t n_levels = 0;
    int64_t n_rows = 0, n_idx = 0, n_coords = 0;
    get(f, &n_levels, 1);
    get(f, &n_rows, 1);
    get(f, &n_idx, 1);
    if (n_levels < 0 || n_levels > gt::MAX_LEVELS || n_rows < 0 || n_idx < 0) die("bad header");
    std::vector<std::vector<int32_t>> off(n_levels);
    for (auto& o : off) {
        int64_t len = 0;
        get(f, &len, 1);
        o.resize((size_t)len);
        get(f, o.data(), o.size());
    }
    get(f, &n_coords, 1);
    std::vector<gt::Bits16> xy((size_t)n_coords);
    get(f, xy.data(), xy.size());
    std::vector<int64_t> idx((size_t)n_idx);
    get(f, idx.data(), idx.size());
    fclose(f);

    // count, scan
    const int32_t* levels[gt::MAX_LEVELS] = {nullptr, nullptr, nullptr};
    for (int l = 0; l < n_levels; ++l) levels[l] = off[l].data();
    std::vector<std::vector<int32_t>> src_lo(n_levels, std::vector<int32_t>((size_t)n_idx)), dst_lo(n_levels, std::vector<int32_t>((size_t)n_idx + 1));
    std::vector<uint8_t> in_range((size_t)n_idx);
    std::vector<int64_t> total(n_levels + 1, 0);
    for (int64_t i = 0; i < n_idx; ++i) {
        const int64_t j = idx[i];
        in_range[i] = j >= 0 && j < n_rows;
        int32_t lo[gt::MAX_LEVELS] = {0, 0, 0}, hi[gt::MAX_LEVELS] = {0, 0, 0};
        if (in_range[i]) gt::row_ranges(levels, n_levels, j, lo, hi);
        for (int l = 0; l < n_levels; ++l) {
            src_lo[l][i] = lo[l];
            dst_lo[l][i] = (int32_t)total[l];
            total[l] += hi[l] - lo[l];
        }
    }
    for (int l = 0; l < n_levels; ++l) dst_lo[l][n_idx] = (int32_t)total[l];

    // fill
    std::vector<std::vector<int32_t>> out_off(n_levels);
    std::vector<gt::Bits16> out_xy;
    if (n_levels == 0) {
        out_xy.resize((size_t)n_idx);
        for (int64_t i = 0; i < n_idx; ++i)
            out_xy[i] = in_range[i] ? xy[(size_t)idx[i]] : gt::Bits16{0x7FF8000000000000ull, 0x7FF8000000000000ull};
    } else {
        out_off[0] = dst_lo[0];
        for (int l = 1; l < n_levels; ++l) {
            out_off[l].assign((size_t)total[l - 1] + 1, -1);
            out_off[l][(size_t)total[l - 1]] = (int32_t)total[l];
            if (n_idx > 0) {
                const gt::OffsetPayload p{off[l].data(), out_off[l].data(), src_lo[l - 1].data(), src_lo[l].data(), dst_lo[l].data()};
                fill(p, dst_lo[l - 1], n_idx, total[l - 1]);
            }
        }
        out_xy.resize((size_t)total[n_levels - 1]);
        if (n_idx > 0) {
            const gt::CoordPayload p{xy.data(), out_xy.data(), src_lo[n_levels - 1].data()};
            fill(p, dst_lo[n_levels - 1], n_idx, total[n_levels - 1]);
        }
    }

    FILE* g = fopen(argv[2], "wb");
    if (!g) die("cannot open the output");
    for (auto& o : out_off) {
        const int64_t len = (int64_t)o.size();
        put(g, &len, 1);
        put(g, o.data(), o.size());
    }
    const int64_t n_out = (int64_t)out_xy.size();
    put(g, &n_out, 1);
    put(g, out_xy.data(), out_xy.size());
    put(g, in_range.data(), in_range.size());
    fclose(g);
    return 0;
}
