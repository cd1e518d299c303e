// gpk_crs.hip — gpk_reproject: analytic reprojection of every coordinate of a column between the systems of gpk_crs.h
// (geographic, Web Mercator, Mercator, transverse Mercator / UTM on WGS84).  One launch, one pass: 16 B in, 16 B out per
// coordinate, the geographic intermediate in registers.  Unlike the affine stream this kernel is bound by f64 arithmetic
// (DESIGN.md section 4.3j has the instruction counts per instance).
#include "gpk_common.h"
#include "gpk_crs.h"

using namespace gpk;

namespace {

// one instance per (source kind, destination kind): no lane branches on the CRS.  Failures are counted per wave — the loop is
// wave-uniform, so the ballot sees every lane — and added once per wave by lane 0 with a vector atomic.
template <int SK, int DK>
__global__ __launch_bounds__(256) void crs_kernel(const double2* __restrict__ xy, int64_t n, gpk_crs_params P, double2* __restrict__ out,
                                                  unsigned long long* __restrict__ n_failed) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long failed = 0;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); i0 < n; i0 += stride) {
        const int64_t i = i0 + lane;
        bool bad = false;
        if (i < n) {
            const double2 p = xy[i];
            double2 q;
            bad = !gpk_crs_transform<SK, DK>(P, p.x, p.y, &q.x, &q.y);
            out[i] = q;
        }
        failed += (unsigned long long)__popcll(__ballot(bad));
    }
    if (n_failed && lane == 0 && failed) atomicAdd(n_failed, failed);
}

struct Launch {
    const double2* xy;
    int64_t n;
    gpk_crs_params P;
    double2* out;
    unsigned long long* n_failed;
    unsigned blocks;
    hipStream_t s;
    int32_t rc = GPK_OK;
    template <int SK, int DK>
    void operator()() {
        rc = [&]() -> int32_t {
            GPK_LAUNCH("gpk_reproject", (crs_kernel<SK, DK>), dim3(blocks), dim3(256), 0, s, xy, n, P, out, n_failed);
            return GPK_OK;
        }();
    }
};

}  // namespace

extern "C" {

int32_t gpk_crs_supported(int32_t epsg) {
    double lon0, fe, fn;
    return gpk_crs_describe(epsg, &lon0, &fe, &fn) >= 0 ? 1 : 0;
}

int32_t gpk_reproject(const gpk_geoarray* a, int32_t src_epsg, int32_t dst_epsg, double* out_xy, int64_t* n_failed, int32_t out_space, void* stream) {
    gpk_crs_params P;
    int sk, dk;
    if (!gpk_crs_make_params(src_epsg, dst_epsg, &P, &sk, &dk))
        return fail(GPK_ERR_INVALID_ARGUMENT, "reproject: EPSG:%d is not supported (4326, 3857, 3395, 32601-32660, 32701-32760 are)",
                    (int)(sk < 0 ? src_epsg : dst_epsg));
    if (!a) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    const int64_t n = a->d.n_coords;
    if (n_failed) *n_failed = 0;
    if (n == 0) return GPK_OK;
    if (!out_xy) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const size_t ob = sizeof(double) * 2 * (size_t)n;
    if (src_epsg == dst_epsg) return copy_out(out_xy, out_space, a->d.xy, ob, s);  // same -> same is a copy
    const bool stage = out_space != GPK_MEM_DEVICE;
    Scratch sc(workspace());
    double* out_dev;
    unsigned long long* cnt;
    sc.stage(out_dev, out_xy, out_space, 2 * (size_t)n);
    sc.add_if(n_failed != nullptr, cnt, 1);
    GPK_TRY(sc.commit());
    if (n_failed) GPK_HIP(hipMemsetAsync(cnt, 0, sizeof *cnt, s));
    int64_t blocks = (n + 255) / 256;
    const int64_t cap = (int64_t)cu_count() * 8;
    if (blocks > cap) blocks = cap;
    Launch l{a->d.xy, n, P, (double2*)out_dev, cnt, (unsigned)blocks, s};
    if (!gpk_crs_dispatch(sk, dk, l)) return fail(GPK_ERR_INVALID_ARGUMENT, "reproject: no instance for kinds %d -> %d", sk, dk);
    GPK_TRY(l.rc);
    if (n_failed) {
        unsigned long long c = 0;
        GPK_HIP(d2h_small(&c, cnt, sizeof c, s));
        if (stage) {
            GPK_HIP(hipMemcpyAsync(out_xy, out_dev, ob, hipMemcpyDeviceToHost, s));
        }
        GPK_HIP(sync_small(s));
        *n_failed = (int64_t)c;
        return GPK_OK;
    }
    return copy_out(out_xy, out_space, out_dev, ob, s);
}

}  // extern "C"
