// Stand-alone host program over csrc/gpk_crs.h: runs the very functions the GPU kernel runs, on the CPU.
//   crs_host_driver IN OUT
// IN is a sequence of records { int32 src_epsg, int32 dst_epsg, int64 n, double xy[2 n] }; for each, OUT receives
// { int64 n_failed, double xy[2 n] }.  Built by tests/test_crs_host.py with the host compiler, once plain and once with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpk_crs.h"

namespace {
struct Run {
    const gpk_crs_params* P;
    const double* in;
    double* out;
    int64_t n, failed = 0;
    template <int SK, int DK>
    void operator()() {
        for (int64_t i = 0; i < n; ++i)
            if (!gpk_crs_transform<SK, DK>(*P, in[2 * i], in[2 * i + 1], &out[2 * i], &out[2 * i + 1])) ++failed;
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t head[2];
    while (fread(head, sizeof head, 1, fi) == 1) {
        int64_t n;
        if (fread(&n, sizeof n, 1, fi) != 1 || n < 0) return 3;
        std::vector<double> in(2 * (size_t)n), out(2 * (size_t)n);
        if (n && fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 3;
        gpk_crs_params P;
        int sk, dk;
        if (!gpk_crs_make_params(head[0], head[1], &P, &sk, &dk)) return 4;
        Run r{&P, in.data(), out.data(), n};
        if (head[0] == head[1])
            out = in;  // same -> same is a copy
        else if (!gpk_crs_dispatch(sk, dk, r))
            return 5;
        fwrite(&r.failed, sizeof r.failed, 1, fo);
        if (n) fwrite(out.data(), sizeof(double), out.size(), fo);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 6;
}
