// gpk_frechet.hip — row-wise discrete Frechet distance between two LINESTRING columns (gpk_frechet_distance).  The cell rules and the
// description of the skewed wavefront are in gpk_frechet.h, the contract in include/geopolars_hip.h.
#include "gpk_frechet.h"
#include "gpk_pairdist.h"

namespace gpk {

namespace {

// The table of one row by G consecutive lanes (a whole wave for G = 64).  W: the walked side, R samples from coordinate wc0; S: the
// side across the lanes, C samples from coordinate sc0; R <= C is the caller's choice, not a requirement.  bcol: at least R doubles of
// LDS that this group owns (touched only when C > G).  Returns the squared value on every lane of the group.
template <int G>
__device__ inline double frechet_table(const double2* __restrict__ xy_w, int64_t wc0, int64_t R, const double2* __restrict__ xy_s, int64_t sc0, int64_t C,
                                       int k, int lane, double* bcol) {
    double answer = 0.0;
    for (int64_t j0 = 0; j0 < C; j0 += G) {
        const int64_t j = j0 + lane;
        const bool col = j < C;
        const bool first = j0 == 0, last = j0 + G >= C;
        double sx = 0.0, sy = 0.0;  // this lane's sample of S
        if (col) {
            const int64_t c = j / k;
            const int jj = (int)(j - c * k);
            const double2 p = xy_s[sc0 + c];
            sx = p.x;
            sy = p.y;
            if (jj > 0) {
                const double2 q = xy_s[sc0 + c + 1];
                sx = fr::sample_coord(p.x, fr::seg_step(p.x, q.x, k), jj);
                sy = fr::sample_coord(p.y, fr::seg_step(p.y, q.y, k), jj);
            }
        }
        double cur = INFINITY;                                // this lane's latest cell: c(i - 1, j) for the next one
        double diag = (first && lane == 0) ? 0.0 : INFINITY;  // c(i - 1, j - 1); the cell above-left of (0, 0) is 0
        double wx = 0.0, wy = 0.0;                            // the walked sample this lane holds (shift register)
        // the walked side's sample generator (group-uniform): sample t is slot wj of coordinate wc
        int64_t wc = wc0;
        int wj = 0;
        double2 wp = xy_w[wc0], wq = wp;
        double stx = 0.0, sty = 0.0;
        const int64_t steps = R + G - 1;
        for (int64_t t = 0; t < steps; ++t) {
            double nx = 0.0, ny = 0.0;
            if (t < R) {
                if (wj == 0 && t + 1 < R) {  // (the coordinate after wc exists)
                    wq = xy_w[wc + 1];
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
            const double lx = __shfl_up(wx, 1, G), ly = __shfl_up(wy, 1, G), lc = __shfl_up(cur, 1, G);
            wx = lane == 0 ? nx : lx;
            wy = lane == 0 ? ny : ly;
            const int64_t i = t - lane;
            double left = lc;
            if (lane == 0) left = (!first && i < R) ? bcol[i] : INFINITY;
            if (col && i >= 0 && i < R) {
                cur = fr::cell(fr::dist2(wx, wy, sx, sy), cur, left, diag);
                if (lane == G - 1 && !last) bcol[i] = cur;
                if (i == R - 1 && j == C - 1) answer = cur;
            }
            diag = left;
        }
        // the boundary column is complete before the next strip reads it: LDS operations of one wave complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    return __shfl(answer, (int)((C - 1) % G), G);
}

// the two rows of a pair and which of them is walked (the shorter one: the boundary column stays small)
struct FrPair {
    int64_t wc0, R, sc0, C;
    const double2 *xy_w, *xy_s;
};
__device__ __forceinline__ FrPair fr_pair(const DevGeo& ga, int64_t ia, const DevGeo& gb, int64_t ib, int k) {
    const int64_t a0 = ga.geom_off[ia], b0 = gb.geom_off[ib];
    const int64_t sa = fr::sample_count(ga.geom_off[ia + 1] - a0, k), sb = fr::sample_count(gb.geom_off[ib + 1] - b0, k);
    if (sa <= sb) return FrPair{a0, sa, b0, sb, ga.xy, gb.xy};
    return FrPair{b0, sb, a0, sa, gb.xy, ga.xy};
}

// One lane group per row and no row loop: nothing (the boundary column included) is carried from row to row.
template <int G>
__global__ __launch_bounds__(256) void frechet_kernel(DevGeo ga, DevGeo gb, const uint32_t* __restrict__ rows, int64_t n, int k, double* __restrict__ out,
                                                      uint32_t* __restrict__ large_rows, uint32_t* __restrict__ n_large, unsigned long long* __restrict__ n_over) {
    __shared__ double bcol[256 / G][fr::FR_GROUP_SHORT];
    const int lane = threadIdx.x & (G - 1), group = threadIdx.x / G;
    const int64_t i = (int64_t)blockIdx.x * (256 / G) + group;
    if (i >= n) return;
    const int64_t ib = rows ? (int64_t)rows[i] : i;
    double d = NAN;
    if (dev::row_ok(ga, i) && dev::row_ok(gb, ib)) {
        const FrPair p = fr_pair(ga, i, gb, ib, k);
        if (p.R > 0) {
            if (p.R > fr::MAX_SHORT) {
                if (lane == 0 && n_over) atomicAdd(n_over, 1ull);
            } else if (p.R * p.C > fr::FR_LARGE_COST) {  // (R <= 2^14 and C < 2^43: no overflow)
                if (lane == 0) large_rows[atomicAdd(n_large, 1u)] = (uint32_t)i;
                return;
            } else {
                d = fr::result(frechet_table<G>(p.xy_w, p.wc0, p.R, p.xy_s, p.sc0, p.C, k, lane, bcol[group]));
            }
        }
    }
    if (lane == 0) out[i] = d;
}

// The listed rows, one wave (the whole work-group) per row: gpk_frechet.h says why.
__global__ __launch_bounds__(64) void frechet_large_kernel(DevGeo ga, DevGeo gb, const uint32_t* __restrict__ rows, int k, const uint32_t* __restrict__ large_rows,
                                                           const uint32_t* __restrict__ n_large, double* __restrict__ out) {
    __shared__ double bcol[fr::MAX_SHORT];
    const uint32_t count = *n_large;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const int64_t i = large_rows[e];
        const int64_t ib = rows ? (int64_t)rows[i] : i;
        const FrPair p = fr_pair(ga, i, gb, ib, k);
        const double c = frechet_table<64>(p.xy_w, p.wc0, p.R, p.xy_s, p.sc0, p.C, k, (int)threadIdx.x, bcol);
        if (threadIdx.x == 0) out[i] = fr::result(c);
    }
}

constexpr unsigned FR_LIST_BLOCKS = 1024;  // four work-groups a compute unit on the 256-CU part this library targets

int32_t frechet_dev(const DevGeo& a, const DevGeo& b, const uint32_t* rows, int64_t n, int k, double* out, uint32_t* large_rows, uint32_t* n_large,
                    unsigned long long* n_over, hipStream_t s) {
    GPK_HIP(hipMemsetAsync(n_large, 0, sizeof(uint32_t), s));
    const int G = pairdist_group_size(a, b);
    // exactly one lane group per row: ceil(n / (256 / G)) blocks, no cap and no row loop in the kernel
    const int64_t per_block = 256 / G;
    const dim3 grid((unsigned)((n + per_block - 1) / per_block)), block(256);
    if (G == 8)
        GPK_LAUNCH("gpk_frechet", (frechet_kernel<8>), grid, block, 0, s, a, b, rows, n, k, out, large_rows, n_large, n_over);
    else
        GPK_LAUNCH("gpk_frechet", (frechet_kernel<32>), grid, block, 0, s, a, b, rows, n, k, out, large_rows, n_large, n_over);
    // the listed rows: a fixed grid of FR_LIST_BLOCKS one-wave work-groups (the device's CU count is not asked) that loops over the list
    // and reads its length on the device; tests/test_gpu_hausdorff.py lists more rows than that, so the loop runs past its first pass
    GPK_LAUNCH("gpk_frechet_large", frechet_large_kernel, dim3(FR_LIST_BLOCKS), dim3(64), 0, s, a, b, rows, k, (const uint32_t*)large_rows,
               (const uint32_t*)n_large, out);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_frechet_distance(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, int32_t subdivisions, double* out,
                                        int64_t* n_over, int32_t out_space, void* stream) {
    if (!a || !b || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_over) *n_over = 0;
    if (subdivisions < 1 || subdivisions > fr::MAX_SUBDIVISIONS)
        return fail(GPK_ERR_INVALID_ARGUMENT, "frechet_distance: subdivisions must be within 1 .. %d (found %d)", fr::MAX_SUBDIVISIONS, (int)subdivisions);
    if (a->d.type != GPK_GEOM_LINESTRING || b->d.type != GPK_GEOM_LINESTRING)
        return fail(GPK_ERR_MISMATCHED_GEOMETRY,
                    "frechet_distance: LINESTRING x LINESTRING only, the measure is defined on one ordered sequence per side (found types %d, %d)", a->d.type,
                    b->d.type);
    if (!b_rows && a->d.n_geoms != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "frechet_distance: row counts differ (%lld vs %lld)", (long long)a->d.n_geoms, (long long)b->d.n_geoms);
    const int64_t n = a->d.n_geoms;
    if (n > (int64_t)INT32_MAX - 1) return fail(GPK_ERR_INVALID_ARGUMENT, "frechet_distance: more than 2^31 - 2 rows");
    GPK_TRY(require_device());
    if (n == 0) return GPK_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t ob = sizeof(double) * (size_t)n;
    const bool host_out = out_space != GPK_MEM_DEVICE;
    Scratch sc(workspace());
    double* out_dev;
    const uint32_t* rows_dev;
    uint32_t *large_rows, *n_large;
    sc.stage(out_dev, out, out_space, (size_t)n);
    sc.stage_in(rows_dev, b_rows, out_space, (size_t)n);
    sc.add(large_rows, (size_t)n);
    sc.add(n_large, 1);
    unsigned long long* cnt;
    sc.add_if(n_over != nullptr, cnt, 1);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    if (n_over) GPK_HIP(hipMemsetAsync(cnt, 0, sizeof *cnt, s));
    GPK_TRY(frechet_dev(a->d, b->d, rows_dev, n, (int)subdivisions, out_dev, large_rows, n_large, cnt, s));
    if (n_over) {  // as n_failed of gpk_reproject: the count is read back, so the call waits for the stream
        unsigned long long c = 0;
        GPK_HIP(d2h_small(&c, cnt, sizeof c, s));
        if (host_out) GPK_HIP(hipMemcpyAsync(out, out_dev, ob, hipMemcpyDeviceToHost, s));
        GPK_HIP(sync_small(s));
        *n_over = (int64_t)c;
        return GPK_OK;
    }
    return sc.copy_back(s);
}
