// Stand-alone host program over the rule of csrc/gpk_triangulate.h: the very routine the GPU lanes run, on one lane (tri::SeqCtx).
//   triangulate_host_driver IN OUT
// IN is a sequence of rows: int32 multi (0: a POLYGON row, 1: a MULTIPOLYGON row), int32 n_members (-1: a null row; a POLYGON row has
// one), per member int32 n_rings, per ring int32 n and double xy[2 n].
// OUT receives per row int32 status (GPK_TRI_*), int32 n_triangles, uint32 index[3 n_triangles] (the row's first coordinate is 0).
// The node lists and the triangle buffer are allocated at exactly the row's share, n_coords + 3 n_rings, so that the sanitized build
// sees any step past it; the program exits with 4 when a row reports more triangles than its share.
// Built by tests/test_triangulate_host.py with the host compiler, once plain and once with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpk_triangulate.h"

namespace tri = gpk::tri;

namespace {
template <typename T>
bool rd(FILE* f, T& v) {
    return fread(&v, sizeof v, 1, f) == 1;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t multi;
    while (rd(fi, multi)) {
        int32_t nm;
        if (!rd(fi, nm) || nm < -1) return 3;
        std::vector<tri::P2> xy;
        std::vector<int32_t> ring_off{0}, part_off{0};
        for (int m = 0; m < nm; ++m) {
            int32_t nr;
            if (!rd(fi, nr) || nr < 0) return 3;
            for (int s = 0; s < nr; ++s) {
                int32_t n;
                if (!rd(fi, n) || n < 0) return 3;
                const size_t at = xy.size();
                xy.resize(at + (size_t)n);
                if (n && fread(xy.data() + at, sizeof(tri::P2), (size_t)n, fi) != (size_t)n) return 3;
                ring_off.push_back((int32_t)xy.size());
            }
            part_off.push_back((int32_t)ring_off.size() - 1);
        }
        int32_t status = GPK_TRI_EMPTY, nt = 0;
        std::vector<uint32_t> out;
        if (nm >= 0) {
            const int n_rings = (int)ring_off.size() - 1;
            const int cap = tri::row_share((int)xy.size(), n_rings);
            std::vector<tri::P2> nxy((size_t)cap);
            std::vector<int> prv((size_t)cap), nxt((size_t)cap), cix((size_t)cap), tag((size_t)cap);
            out.resize(3 * (size_t)cap);
            const tri::Nodes nd{nxy.data(), prv.data(), nxt.data(), cix.data(), tag.data()};
            const tri::RowView r{xy.data(), ring_off.data(), multi ? part_off.data() : nullptr, 0, multi ? nm : 0, 0, n_rings};
            int n = 0;
            status = tri::triangulate_row(r, nd, cap, out.data(), tri::SeqCtx{0}, n);
            if (n > cap) return 4;
            nt = status == GPK_TRI_OK ? n : 0;
        }
        if (fwrite(&status, sizeof status, 1, fo) != 1 || fwrite(&nt, sizeof nt, 1, fo) != 1) return 6;
        if (nt && fwrite(out.data(), sizeof(uint32_t), 3 * (size_t)nt, fo) != 3 * (size_t)nt) return 6;
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 6;
}
