// gpk_gridindex.hip — the spatial index handle and its grid directory (gpk_index.h): boxes, extent, cell -> ascending ids.
//
//   gpk_index_build   == SpatialIndex::try_from(&Series)            spatial_index.rs:320-334
//
// The point-in-polygon tables of a polygonal array are built by gpk_pipindex.hip (build_pip_index) on top of the directory.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "gpk_device.h"
#include "gpk_index.h"
#include "gpk_scan.h"

namespace gpk {

// ================================= index build ==================================================
// stage 1 of the extent: one closed box per work-group (NaN = nothing but empty geometries), in the boxes' own format, so
// that extent_kernel folds them like boxes (min / max are exact: the result does not depend on the split)
__global__ __launch_bounds__(256) void extent_partial_kernel(const double4* __restrict__ bbox, int64_t n, double4* __restrict__ part) {
    __shared__ double red[4][4];
    double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double4 b = bbox[i];
        if (b.x == b.x) {
            mnx = fmin(mnx, b.x);
            mny = fmin(mny, b.y);
            mxx = fmax(mxx, b.z);
            mxy = fmax(mxy, b.w);
        }
    }
    mnx = dev::wave_min(mnx);
    mny = dev::wave_min(mny);
    mxx = dev::wave_max(mxx);
    mxy = dev::wave_max(mxy);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = mnx;
        red[1][wave] = mny;
        red[2][wave] = mxx;
        red[3][wave] = mxy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mnx = fmin(mnx, red[0][w]);
            mny = fmin(mny, red[1][w]);
            mxx = fmax(mxx, red[2][w]);
            mxy = fmax(mxy, red[3][w]);
        }
        part[blockIdx.x] = mnx <= mxx ? make_double4(mnx, mny, mxx, mxy) : make_double4(NAN, NAN, NAN, NAN);
    }
}
__global__ __launch_bounds__(1024) void extent_kernel(const double4* __restrict__ bbox, int64_t n,
                                                      int gx, int gy, GridParams* __restrict__ out) {
    __shared__ double red[4][16];
    double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const double4 b = bbox[i];
        if (b.x == b.x) {  // NaN marks an empty geometry
            mnx = fmin(mnx, b.x);
            mny = fmin(mny, b.y);
            mxx = fmax(mxx, b.z);
            mxy = fmax(mxy, b.w);
        }
    }
    mnx = dev::wave_min(mnx);
    mny = dev::wave_min(mny);
    mxx = dev::wave_max(mxx);
    mxy = dev::wave_max(mxy);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = mnx;
        red[1][wave] = mny;
        red[2][wave] = mxx;
        red[3][wave] = mxy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            mnx = fmin(mnx, red[0][w]);
            mny = fmin(mny, red[1][w]);
            mxx = fmax(mxx, red[2][w]);
            mxy = fmax(mxy, red[3][w]);
        }
        GridParams g;
        const bool any = mnx <= mxx;
        g.x0 = any ? mnx : 0.0;
        g.y0 = any ? mny : 0.0;
        const double w = any ? mxx - mnx : 0.0, h = any ? mxy - mny : 0.0;
        g.inv_w = w > 0.0 ? (double)gx / w : 0.0;
        g.inv_h = h > 0.0 ? (double)gy / h : 0.0;
        g.gx = gx;
        g.gy = gy;
        *out = g;
    }
}

template <bool FILL>
__global__ void grid_register_kernel(const double4* __restrict__ bbox, int64_t n,
                                     const GridParams* __restrict__ gp, int32_t* __restrict__ cell_cnt,
                                     int32_t* __restrict__ items) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double4 b = bbox[j];
    if (!(b.x == b.x)) return;
    const GridParams g = *gp;
    const int cx0 = dev::cell_of(b.x, g.x0, g.inv_w, g.gx), cx1 = dev::cell_of(b.z, g.x0, g.inv_w, g.gx);
    const int cy0 = dev::cell_of(b.y, g.y0, g.inv_h, g.gy), cy1 = dev::cell_of(b.w, g.y0, g.inv_h, g.gy);
    for (int cy = cy0; cy <= cy1; ++cy)
        for (int cx = cx0; cx <= cx1; ++cx) {
            const int c = cy * g.gx + cx;
            const int slot = atomicAdd(&cell_cnt[c], 1);
            if (FILL) items[slot] = (int32_t)j;
        }
}

// ascending ids within each cell -> deterministic candidate order, hence sorted (l, r) output
__global__ void cell_sort_kernel(const int32_t* __restrict__ cell_off, int64_t n_cells, int32_t* __restrict__ items) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    const int b = cell_off[c], e = cell_off[c + 1];
    for (int i = b + 1; i < e; ++i) {
        const int32_t key = items[i];
        int k = i - 1;
        while (k >= b && items[k] > key) {
            items[k + 1] = items[k];
            --k;
        }
        items[k + 1] = key;
    }
}

static inline dim3 grid_for(int64_t n, int block) {
    int64_t b = (n + block - 1) / block;
    return dim3((unsigned)(b > 0 ? b : 1));
}

}  // namespace gpk

using namespace gpk;

extern "C" {

int32_t gpk_index_free(gpk_index* idx) {
    if (!idx) return GPK_OK;
    // (hipFree's implicit wait, once: a join enqueued against this index may still be running — on the device that OWNS the tables,
    // which need not be the calling thread's current one: the blocks go back to a process-wide cache tagged by device)
    (void)sync_device(idx->device);
    for (int i = 0; i < 24; ++i)
        if (idx->owned[i]) cached_free(idx->owned[i]);
    delete idx;
    return GPK_OK;
}

int32_t gpk_index_describe(const gpk_index* idx, int64_t out[8]) {
    if (!idx || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = idx->pip.R;
    out[1] = idx->pip_lean;
    out[2] = idx->pip.chain_xy != nullptr;
    out[3] = idx->pip.route != nullptr;
    out[4] = idx->pip_list_heavy;
    out[5] = idx->route_own;
    out[6] = idx->route_single;
    return GPK_OK;
}

int32_t gpk_index_nbytes(const gpk_index* idx, int64_t* out_bytes) {
    if (!idx || !out_bytes) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_bytes = idx->nbytes;
    return GPK_OK;
}

int32_t gpk_index_build(const gpk_geoarray* a, void* stream, gpk_index** out) {
    return gpk_index_build_ex(a, GPK_INDEX_BBOX_GRID | GPK_INDEX_PIP, nullptr, stream, out);
}

int32_t gpk_index_build_ex(const gpk_geoarray* a, int32_t parts, const double* bbox4_dev, void* stream, gpk_index** out) {
    if (!a || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = a->d.n_geoms;

    gpk_index* ix = new gpk_index;
    memset(ix, 0, sizeof *ix);
    ix->device = a->device;
    ix->n_geoms = n;
    ix->geom_type = a->d.type;
    ix->n_coords = a->d.n_coords;
    ix->n_rings = a->d.n_rings;
    {
        static std::atomic<uint64_t> next_serial{1};
        ix->serial = next_serial.fetch_add(1);
    }

    // grid resolution: ~2 cells per geometry along each axis of a square layout
    int gdim = (int)ceil(2.0 * sqrt((double)(n > 0 ? n : 1)));
    if (gdim < 1) gdim = 1;
    if (gdim > 2048) gdim = 2048;
    const int64_t n_cells = (int64_t)gdim * gdim;

    auto cleanup = [&](int32_t rc) {
        gpk_index_free(ix);
        return rc;
    };
#define IX_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return cleanup(fail(_e == hipErrorOutOfMemory ? GPK_ERR_OOM : GPK_ERR_DEVICE,         \
                                "%s failed: %s", #expr, hipGetErrorString(_e)));                  \
    } while (0)
#define IX_TRY(expr)                             \
    do {                                         \
        int32_t _rc = (expr);                    \
        if (_rc != GPK_OK) return cleanup(_rc);  \
    } while (0)

    const bool dbg_time = getenv("GPK_DEBUG_INDEX") != nullptr;  // wall time of the directory phases (the stream is drained per stamp)
    auto t_last = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what) {
        if (!dbg_time) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[gpk] index build: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    double4* bbox = nullptr;
    GridParams* grid = nullptr;
    int32_t* cell_off = nullptr;
    IX_HIP(cached_malloc((void**)&bbox, sizeof(double4) * (size_t)(n > 0 ? n : 1)));
    ix->owned[0] = bbox;
    IX_HIP(cached_malloc((void**)&grid, sizeof(GridParams)));
    ix->owned[1] = grid;
    IX_HIP(cached_malloc((void**)&cell_off, sizeof(int32_t) * (size_t)(n_cells + 1)));
    ix->owned[2] = cell_off;

    // 1. bounding boxes (NodeEnvelope, spatial_index.rs:212-312) — or the caller's (the leaves another rank built and
    //    sent over xGMI: dist.all_gather_leaves)
    if (bbox4_dev)
        IX_HIP(hipMemcpyAsync(bbox, bbox4_dev, sizeof(double4) * (size_t)n, hipMemcpyDeviceToDevice, s));
    else
        IX_TRY(gpk_bounds(a, (double*)bbox, GPK_MEM_DEVICE, stream));

    stamp("boxes (gpk_bounds)");
    // 2. extent + grid parameters, all on device (two stages beyond a few thousand boxes: one work-group walked 5M of them in 4.7 ms)
    const int64_t n_blocks = (n_cells + 255) / 256;
    const int64_t ext_blocks = n > 65536 ? 1024 : 0;
    Scratch sc(workspace());
    int32_t *cell_cnt, *cursor;
    unsigned long long* btot;
    double4* ext_part;
    sc.add_n((size_t)(n_cells + 1), cell_cnt, cursor);
    sc.add(btot, (size_t)(n_blocks + 1));
    sc.add(ext_part, 1024);
    IX_TRY(sc.commit());
    if (ext_blocks) {
        GPK_LAUNCH_OR(cleanup, "gpk_index_extent_partial", extent_partial_kernel, dim3((unsigned)ext_blocks), dim3(256), 0, s, bbox, n, ext_part);
        GPK_LAUNCH_OR(cleanup, "gpk_index_extent", extent_kernel, dim3(1), dim3(1024), 0, s, (const double4*)ext_part, ext_blocks, gdim, gdim, grid);
    } else {
        GPK_LAUNCH_OR(cleanup, "gpk_index_extent", extent_kernel, dim3(1), dim3(1024), 0, s, bbox, n, gdim, gdim, grid);
    }

    stamp("extent");
    // 3. count, scan, fill, sort
    IX_HIP(hipMemsetAsync(cell_cnt, 0, sizeof(int32_t) * (size_t)(n_cells + 1), s));
    if (n > 0)
        GPK_LAUNCH_OR(cleanup, "gpk_index_count", grid_register_kernel<false>, grid_for(n, 256), dim3(256), 0, s, bbox, n, grid, cell_cnt, (int32_t*)nullptr);
    IX_TRY(exclusive_scan_i32(cell_cnt, n_cells, cell_off, cursor, btot, s));
    unsigned long long total = 0;
    IX_HIP(d2h_small(&total, btot + n_blocks, sizeof total, s));
    IX_HIP(d2h_small(&ix->host_grid, grid, sizeof(GridParams), s));
    IX_HIP(sync_small(s));
    if (total > (unsigned long long)INT32_MAX)
        return cleanup(fail(GPK_ERR_INVALID_OFFSETS, "spatial index directory overflows i32 (%llu entries)", total));
    int32_t* items = nullptr;
    IX_HIP(cached_malloc((void**)&items, sizeof(int32_t) * (size_t)(total > 0 ? total : 1)));
    ix->owned[3] = items;
    if (n > 0) {
        GPK_LAUNCH_OR(cleanup, "gpk_index_fill", grid_register_kernel<true>, grid_for(n, 256), dim3(256), 0, s, bbox, n, grid, cursor, items);
        GPK_LAUNCH_OR(cleanup, "gpk_index_sort", cell_sort_kernel, grid_for(n_cells, 256), dim3(256), 0, s, cell_off, n_cells, items);
    }
    IX_HIP(hipStreamSynchronize(s));  // the workspace may be recycled by the next call on another stream
    stamp("directory");
#undef IX_HIP
#undef IX_TRY

    ix->v.bbox = bbox;
    ix->v.grid = grid;
    ix->v.cell_off = cell_off;
    ix->v.items = items;
    ix->v.gx = gdim;
    ix->v.gy = gdim;
    ix->nbytes = (int64_t)(sizeof(double4) * (size_t)n + sizeof(GridParams) + sizeof(int32_t) * (size_t)(n_cells + 1) +
                           sizeof(int32_t) * (size_t)total);
    if (parts & GPK_INDEX_PIP) {
        const int32_t rc = build_pip_index(a, ix, s, (parts & GPK_INDEX_PIP_LIGHT) ? 0 : ((parts & GPK_INDEX_PIP_FULL) ? 2 : 1));  // raster + slabs for polygonal arrays
        if (rc != GPK_OK) {
            gpk_index_free(ix);
            return rc;
        }
    }
    *out = ix;
    return GPK_OK;
}

}  // extern "C"
