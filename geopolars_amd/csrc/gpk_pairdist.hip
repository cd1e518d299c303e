// gpk_pairdist.hip — row-wise Euclidean distance between two non-point geometry columns.
//   geoseries.rs:141-146 (GeoSeries::distance) for the pairs of {MULTIPOINT, LINESTRING, MULTILINESTRING, POLYGON, MULTIPOLYGON};
//   upstream: geo 0.27 EuclideanDistance.  Pairs with a POINT column stay in gpk_rowwise.hip.
//
// Per row (A = a[i], B = b[b_rows[i]] or b[i]):
//   null or empty side               -> NaN (empty: no member has a coordinate; empty members of a multi-geometry are ignored)
//   A and B intersect (closed sets)  -> 0.0 exactly, decided with exact orientations:
//       a vertex of one side inside or on a polygonal other side (holes excluded), or
//       a segment of A meets a segment of B (line_intersects_line: touching and collinear overlap count)
//   otherwise                        -> min over every vertex of one side and every segment of the other, both ways, of the
//                                       point-segment distance, compared exactly as fractions; one square root at the end.
// Every coordinate c of a row defines one segment: (c, c + 1) when c + 1 lies in the same sequence, else the degenerate (c, c).
// A one-coordinate sequence and a MULTIPOINT member are therefore degenerate segments, as the contract asks; the degenerate
// segment at the last coordinate of a longer sequence changes nothing (its distances are never below those of the segment
// that ends there, and its point lies on that segment).
//
// Schedules.  Rows cost about n_A * n_B (coordinates of both sides):
//   pairdist_kernel<G, KA, KB>      G lanes per row.  Lanes stride over the coordinates of the longer side while the group walks
//                                   the shorter one; the crossing test runs only on segment pairs whose boxes meet, and the group
//                                   stops as soon as a lane proves an intersection.  Rows above PD_LARGE_COST are appended to a
//                                   list instead.
//   pairdist_large_kernel<KA, KB>   one 256-lane work-group per listed row; the shorter side is staged in LDS in chunks of
//                                   PDL_CHUNK segments, every thread strides over the longer side.  Launched with a fixed grid
//                                   that reads the list's length on the device: no read-back, results stay stream-ordered.
// The kernels are instantiated for KA <= KB (15 unordered pairs); the dispatch swaps the columns when a's family code is the
// larger one, so distance(a, b) and distance(b, a) evaluate the same pairs in the same order.
#include "gpk_pairdist.h"

namespace gpk {

template <int KA, int KB>
__device__ __forceinline__ void pair_rows(const DevGeo& ga, const DevGeo& gb, const uint32_t* __restrict__ rows, bool swapped, int64_t i,
                                          int64_t& ia, int64_t& ib) {
    const int64_t j = rows ? (int64_t)rows[i] : i;
    ia = swapped ? j : i;
    ib = swapped ? i : j;
}

// G lanes per row; rows above PD_LARGE_COST are listed for pairdist_large_kernel.  (ga, gb) are the columns in canonical order
// (KA <= KB); `swapped`: gb is the caller's left column, so the row map indexes ga.
template <int G, int KA, int KB>
__global__ __launch_bounds__(256) void pairdist_kernel(DevGeo ga, DevGeo gb, const uint32_t* __restrict__ rows, bool swapped, int64_t n,
                                                       double* __restrict__ out, uint32_t* __restrict__ large_rows,
                                                       uint32_t* __restrict__ n_large) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += groups) {
        int64_t ia, ib;
        pair_rows<KA, KB>(ga, gb, rows, swapped, i, ia, ib);
        double d = NAN;
        if (dev::row_ok(ga, ia) && dev::row_ok(gb, ib)) {
            const RowSeqs a = row_seqs<KA>(ga, ia), b = row_seqs<KB>(gb, ib);
            const int na = a.c1 - a.c0, nb = b.c1 - b.c0;
            if (na > 0 && nb > 0) {
                if ((int64_t)na * nb > PD_LARGE_COST) {
                    if (lane == 0) large_rows[atomicAdd(n_large, 1u)] = (uint32_t)i;
                    continue;
                }
                d = pair_distance_group<G, KA, KB>(ga, ia, a, gb, ib, b, lane);
            }
        }
        if (lane == 0) out[i] = d;
    }
}

// One 256-lane work-group per listed row (pair_distance_workgroup, gpk_pairdist.h).
template <int KA, int KB>
__global__ __launch_bounds__(256) void pairdist_large_kernel(DevGeo ga, DevGeo gb, const uint32_t* __restrict__ rows, bool swapped,
                                                             const uint32_t* __restrict__ large_rows, const uint32_t* __restrict__ n_large,
                                                             double* __restrict__ out) {
    __shared__ PairLargeLds lds;
    const uint32_t count = *n_large;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const int64_t i = large_rows[e];
        int64_t ia, ib;
        pair_rows<KA, KB>(ga, gb, rows, swapped, i, ia, ib);
        const double d = pair_distance_workgroup<KA, KB>(ga, ia, gb, ib, lds);
        if (threadIdx.x == 0) out[i] = d;
    }
}

template <int KA, int KB>
static int32_t pairdist_launch(const DevGeo& ga, const DevGeo& gb, const uint32_t* rows, bool swapped, int64_t n, double* out,
                               uint32_t* large_rows, uint32_t* n_large, hipStream_t s) {
    const int G = pairdist_group_size(ga, gb);
    const int64_t per_block = 256 / G;
    int64_t blocks = (n + per_block - 1) / per_block;
    if (blocks > (int64_t)cu_count() * 16) blocks = (int64_t)cu_count() * 16;
    const dim3 grid((unsigned)blocks), block(256);
    if (G == 8)
        GPK_LAUNCH("gpk_pairdist", (pairdist_kernel<8, KA, KB>), grid, block, 0, s, ga, gb, rows, swapped, n, out, large_rows, n_large);
    else
        GPK_LAUNCH("gpk_pairdist", (pairdist_kernel<32, KA, KB>), grid, block, 0, s, ga, gb, rows, swapped, n, out, large_rows, n_large);
    // the listed rows: a fixed grid that reads the list's length on the device (idle work-groups return at once)
    const int64_t lb = (int64_t)cu_count() * 4 < n ? (int64_t)cu_count() * 4 : n;
    GPK_LAUNCH("gpk_pairdist_large", (pairdist_large_kernel<KA, KB>), dim3((unsigned)lb), block, 0, s, ga, gb, rows, swapped,
               (const uint32_t*)large_rows, (const uint32_t*)n_large, out);
    return GPK_OK;
}

// Row-wise distance for two non-point columns (gpk_distance_rowwise).  rows: device, or nullptr; out: device, n = rows of a.
int32_t pair_distance_dev(const DevGeo& a, const DevGeo& b, const uint32_t* rows, int64_t n, double* out, uint32_t* large_rows,
                          uint32_t* n_large, hipStream_t s) {
    GPK_HIP(hipMemsetAsync(n_large, 0, sizeof(uint32_t), s));
    const bool swapped = a.type > b.type;
    const DevGeo& ga = swapped ? b : a;
    const DevGeo& gb = swapped ? a : b;
    constexpr int MP = GPK_GEOM_MULTIPOINT, LS = GPK_GEOM_LINESTRING, MLS = GPK_GEOM_MULTILINESTRING, PG = GPK_GEOM_POLYGON,
                  MPG = GPK_GEOM_MULTIPOLYGON;
#define PD(KA, KB)                                                                                         \
    if (ga.type == KA && gb.type == KB) return pairdist_launch<KA, KB>(ga, gb, rows, swapped, n, out, large_rows, n_large, s)
    PD(LS, LS); PD(LS, PG); PD(LS, MP); PD(LS, MLS); PD(LS, MPG);
    PD(PG, PG); PD(PG, MP); PD(PG, MLS); PD(PG, MPG);
    PD(MP, MP); PD(MP, MLS); PD(MP, MPG);
    PD(MLS, MLS); PD(MLS, MPG);
    PD(MPG, MPG);
#undef PD
    return fail(GPK_ERR_MISMATCHED_GEOMETRY, "distance: no kernel for geometry types %d, %d", a.type, b.type);
}

}  // namespace gpk
