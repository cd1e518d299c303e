// pointrel_host_driver.cpp — the per-pair routine of csrc/gpk_pointrel.h (pt::point_mask_group) run on the CPU at G = 1 with an exact
// __int128 orientation (the fixtures' coordinates are integers).
//   pointrel_host_driver IN OUT
// IN is a sequence of records, one per pair:
//   int32 one (A comes from a POINT column: the one-point instantiation), int32 dim_b (0, 1, 2), int32 n_a, int32 n_seq (sequences of
//   B; 0 for a punctual B), int32 n_b, then n_a points of A (2 doubles each), n_seq + 1 int32 sequence offsets into B's coordinates
//   (only when n_seq > 0), n_b coordinates of B
// OUT receives 10 bytes per record: the full mask, then for each of the nine predicate ids predicate_of(the mask computed with that
// predicate's early stop).  Built by tests/test_pointrel_host.py with the host compiler, once plain and once with
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_pointrel.h"

namespace pt = gpk::pt;

namespace {

struct ExactOrient {
    int operator()(pt::P2 a, pt::P2 b, pt::P2 c) const {
        const __int128 ax = (int64_t)a.x, ay = (int64_t)a.y, bx = (int64_t)b.x, by = (int64_t)b.y, cx = (int64_t)c.x, cy = (int64_t)c.y;
        const __int128 d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
        return d > 0 ? 1 : (d < 0 ? -1 : 0);
    }
};

template <typename T>
bool rd(FILE* f, T& v) {
    return fread(&v, sizeof v, 1, f) == 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t one;
    while (rd(in, one)) {
        int32_t dim_b, n_a, n_seq, n_b;
        if (!rd(in, dim_b) || !rd(in, n_a) || !rd(in, n_seq) || !rd(in, n_b) || n_a < 0 || n_seq < 0 || n_b < 0 || dim_b < 0 || dim_b > 2) return 3;
        std::vector<pt::P2> a((size_t)n_a), b((size_t)n_b);
        std::vector<int32_t> so;
        for (auto& p : a)
            if (!rd(in, p.x) || !rd(in, p.y)) return 3;
        if (n_seq > 0) {
            so.resize((size_t)n_seq + 1);
            for (auto& o : so)
                if (!rd(in, o)) return 3;
            if (so.front() != 0 || so.back() != n_b) return 3;
        } else if (dim_b != 0 && n_b != 0) {
            return 3;
        }
        for (auto& p : b)
            if (!rd(in, p.x) || !rd(in, p.y)) return 3;
        const pt::Row A{a.data(), nullptr, 0, 0, 0, n_a, 0};
        const pt::Row B{b.data(), n_seq > 0 ? so.data() : nullptr, 0, n_seq, 0, n_b, dim_b};
        auto run = [&](pt::Stop st) {
            return one ? pt::point_mask_group<1, true>(A, B, 0, st, ExactOrient{}) : pt::point_mask_group<1, false>(A, B, 0, st, ExactOrient{});
        };
        uint8_t rec[10];
        rec[0] = (uint8_t)run(pt::Stop{0, pt::PT_ALL});
        for (int pred = 0; pred < 9; ++pred) rec[1 + pred] = pt::predicate_of(run(pt::stop_of(pred)), pred, dim_b) ? 1 : 0;
        if (fwrite(rec, 1, sizeof rec, out) != sizeof rec) return 4;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
