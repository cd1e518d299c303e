// gpk_triangulate.hip — gpk_triangulate over the rule of gpk_triangulate.h.  Contract: include/geopolars_hip.h.
//
// A row's triangles are not known before it is clipped, but they are bounded: every row writes into its own SHARE of a scratch index
// buffer (slot c0 + 3 s0 for a row whose first coordinate is c0 and first ring s0), the counts are scanned, the total is read back
// (the one read-back) and a gather moves the shares to their offsets.
//   rows     G lanes a row (4 or 16 by the column's mean share), one group per row on an uncapped grid, the node list in the group's
//            LDS slice (TRI_SLICE_SMALL / TRI_SLICE_LARGE slots of 32 bytes).  A row above the slice is put on a list.
//   large    one work-group of 256 lanes per listed row, the list in LDS (up to TRI_LDS_NODES slots: 160 000 bytes, dynamic).
//   huge     rows above TRI_LDS_NODES slots: the same work-group routine with the list in global scratch — correct and slow.
// Both list kernels are launched with one work-group for every row that COULD be listed (total share / threshold); the others leave at once.
#include "gpk_device.h"
#include "gpk_scan.h"
#include "gpk_triangulate.h"

namespace gpk {

namespace {

constexpr int BT = tri::TRI_BLOCK_THREADS;

template <int G>
struct GroupCtx {
    static constexpr int T = G;
    int lane;
    __device__ __forceinline__ int imin(int v) const { return dev::group_allreduce<G>(v, [](int a, int b) { return a < b ? a : b; }); }
    __device__ __forceinline__ int ior(int v) const { return dev::group_or<G>(v); }
    __device__ __forceinline__ double dmin(double v) const { return dev::group_min<G>(v); }
    __device__ __forceinline__ void sync() const {  // the lanes of a group sit in one wave: a compiler-level fence orders the LDS traffic
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};
struct BlockCtx {
    static constexpr int T = BT;
    int lane;
    int* islot;      // LDS
    double* dslot;   // LDS, BT / 64
    __device__ __forceinline__ int imin(int v) const {
        if (lane == 0) *islot = tri::NONE;
        __syncthreads();
        if (v != tri::NONE) atomicMin(islot, v);
        __syncthreads();
        const int r = *islot;
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ int ior(int v) const {
        if (lane == 0) *islot = 0;
        __syncthreads();
        if (v) atomicOr(islot, v);
        __syncthreads();
        const int r = *islot;
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ double dmin(double v) const {
        const double w = dev::wave_min(v);
        if ((lane & 63) == 0) dslot[lane >> 6] = w;
        __syncthreads();
        double r = dslot[0];
        for (int k = 1; k < BT / 64; ++k) r = fmin(r, dslot[k]);
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

struct RowAt {
    tri::RowView view;
    int share;       // node and triangle slots
    int64_t start;   // first slot of the row in the column-wide share space
};
__device__ __forceinline__ RowAt row_at(const DevGeo& a, int64_t g) {
    RowAt r;
    r.view.xy = reinterpret_cast<const tri::P2*>(a.xy);
    r.view.ring_off = a.ring_off;
    if (a.type == GPK_GEOM_MULTIPOLYGON) {
        r.view.part_off = a.part_off;
        r.view.p0 = a.geom_off[g];
        r.view.p1 = a.geom_off[g + 1];
        r.view.s0 = a.part_off[r.view.p0];
        r.view.s1 = a.part_off[r.view.p1];
    } else {
        r.view.part_off = nullptr;
        r.view.p0 = r.view.p1 = 0;
        r.view.s0 = a.geom_off[g];
        r.view.s1 = a.geom_off[g + 1];
    }
    const int c0 = a.ring_off[r.view.s0], c1 = a.ring_off[r.view.s1];
    r.share = tri::row_share(c1 - c0, r.view.s1 - r.view.s0);
    r.start = (int64_t)c0 + 3 * (int64_t)r.view.s0;
    return r;
}

struct Lists {
    int32_t* big;    // big[0]: rows listed, big[1 ..]: their numbers
    int32_t* huge;
};

// ---- G lanes per row, one group per row ----------------------------------------------------------------------------------------------
template <int G, int SLICE>
__global__ __launch_bounds__(256) void triangulate_rows_kernel(DevGeo a, int64_t n, Lists lists, uint32_t* __restrict__ tris, int32_t* __restrict__ counts,
                                                                uint8_t* __restrict__ status) {
    constexpr int GROUPS = 256 / G;
    __shared__ tri::P2 l_xy[GROUPS][SLICE];
    __shared__ int l_int[GROUPS][4][SLICE];
    const int grp = threadIdx.x / G;
    const GroupCtx<G> cx{(int)(threadIdx.x & (G - 1))};
    const int64_t g = (int64_t)blockIdx.x * GROUPS + grp;
    if (g >= n) return;  // (group-uniform, as is every branch below)
    int st = GPK_TRI_EMPTY, nt = 0;
    if (dev::valid_row(a.validity, g)) {
        const RowAt r = row_at(a, g);
        if (r.share > SLICE) {
            int32_t* list = r.share > tri::TRI_LDS_NODES ? lists.huge : lists.big;
            if (cx.lane == 0) list[1 + atomicAdd(list, 1)] = (int32_t)g;
            return;
        }
        const tri::Nodes nd{l_xy[grp], l_int[grp][0], l_int[grp][1], l_int[grp][2], l_int[grp][3]};
        st = tri::triangulate_row(r.view, nd, r.share, tris + 3 * r.start, cx, nt);
    }
    if (cx.lane == 0) {
        counts[g] = st == GPK_TRI_OK ? nt : 0;
        status[g] = (uint8_t)st;
    }
}

// ---- a work-group per listed row -------------------------------------------------------------------------------------------------------
template <bool GLOBAL>
__global__ __launch_bounds__(BT) void triangulate_list_kernel(DevGeo a, const int32_t* __restrict__ list, char* __restrict__ node_scratch,
                                                              uint32_t* __restrict__ tris, int32_t* __restrict__ counts, uint8_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char l_nodes[];
    __shared__ int islot;
    __shared__ double dslot[BT / 64];
    if ((int)blockIdx.x >= list[0]) return;
    const int64_t g = list[1 + blockIdx.x];
    const BlockCtx cx{(int)threadIdx.x, &islot, dslot};
    const RowAt r = row_at(a, g);
    char* base = GLOBAL ? node_scratch + (size_t)tri::NODE_BYTES * (size_t)r.start : l_nodes;
    const size_t cap = (size_t)r.share;
    int* ints = reinterpret_cast<int*>(base + sizeof(tri::P2) * cap);
    const tri::Nodes nd{reinterpret_cast<tri::P2*>(base), ints, ints + cap, ints + 2 * cap, ints + 3 * cap};
    int nt = 0;
    const int st = tri::triangulate_row(r.view, nd, r.share, tris + 3 * r.start, cx, nt);
    if (cx.lane == 0) {
        counts[g] = st == GPK_TRI_OK ? nt : 0;
        status[g] = (uint8_t)st;
    }
}

// the shares to their offsets: 16 lanes a row
__global__ __launch_bounds__(256) void triangulate_gather_kernel(DevGeo a, int64_t n, const uint32_t* __restrict__ tris, const int32_t* __restrict__ offsets,
                                                                 uint32_t* __restrict__ out) {
    const int lane = threadIdx.x & 15;
    const int64_t g = (int64_t)blockIdx.x * 16 + threadIdx.x / 16;
    if (g >= n) return;
    const int o0 = offsets[g], m = 3 * (offsets[g + 1] - o0);
    if (m == 0) return;
    const uint32_t* __restrict__ src = tris + 3 * row_at(a, g).start;
    for (int k = lane; k < m; k += 16) out[3 * (int64_t)o0 + k] = src[k];
}

int32_t allow_lds(size_t bytes) {
    // (an attribute of the function on the current device: setting it again is harmless and costs no device work)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&triangulate_list_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(GPK_ERR_DEVICE, "triangulate: %zu bytes of LDS refused: %s", bytes, hipGetErrorString(e));
    return GPK_OK;
}

int tri_group_size(int64_t total_share, int64_t n) { return n > 0 && (double)total_share / (double)n >= tri::TRI_G_MEAN ? tri::TRI_G_LARGE : tri::TRI_G_SMALL; }

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_triangulate(const gpk_geoarray* a, uint32_t* out_index, int64_t tri_capacity, int32_t* out_tri_offsets, uint8_t* out_status,
                                   int64_t* n_triangles, int32_t out_space, void* stream) {
    if (!a || !out_tri_offsets || !n_triangles) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_triangles = 0;
    if (!is_polygonal(a->d.type)) return fail(GPK_ERR_MISMATCHED_GEOMETRY, "triangulate: POLYGON | MULTIPOLYGON (found type %d)", a->d.type);
    if (tri_capacity < 0) return fail(GPK_ERR_INVALID_ARGUMENT, "triangulate: tri_capacity %lld", (long long)tri_capacity);
    GPK_TRY(require_device());
    const DevGeo& d = a->d;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = d.n_geoms, total_share = d.n_coords + 3 * d.n_rings;
    const bool host_out = out_space != GPK_MEM_DEVICE;
    if (n > (int64_t)INT32_MAX - 1 || total_share > (int64_t)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "triangulate: more than 2^31 - 2 rows, or n_coords + 3 n_rings above 2^31 - 1: shard the column");
    if (n == 0) {
        if (host_out) {
            out_tri_offsets[0] = 0;
            return GPK_OK;
        }
        GPK_HIP(hipMemsetAsync(out_tri_offsets, 0, sizeof(int32_t), s));
        return GPK_OK;
    }
    const int G = tri_group_size(total_share, n);
    const int slice = G == tri::TRI_G_LARGE ? tri::TRI_SLICE_LARGE : tri::TRI_SLICE_SMALL;
    const bool any_big = total_share > slice, any_huge = total_share > tri::TRI_LDS_NODES;  // (else no row can be listed)
    Scratch sc(workspace());
    int32_t *counts, *offsets_dev;
    Lists lists;
    uint8_t* status_dev;
    unsigned long long* block_tot;
    uint32_t* tris;
    char* node_scratch;
    sc.add(counts, (size_t)(n + 1));
    sc.stage(offsets_dev, out_tri_offsets, out_space, (size_t)(n + 1));
    sc.add_n((size_t)(n + 1), lists.big, lists.huge);
    sc.stage_or_add(status_dev, out_status, out_space, (size_t)n);
    sc.add(block_tot, (size_t)((n + 255) / 256 + 2));
    sc.add(tris, 3 * (size_t)total_share);
    sc.add_if(any_huge, node_scratch, (size_t)tri::NODE_BYTES * (size_t)total_share);
    GPK_TRY(sc.commit());
    GPK_HIP(hipMemsetAsync(lists.big, 0, sizeof(int32_t), s));
    GPK_HIP(hipMemsetAsync(lists.huge, 0, sizeof(int32_t), s));

    const int64_t per_block = 256 / G;
    const dim3 grid((unsigned)((n + per_block - 1) / per_block));
    if (G == tri::TRI_G_LARGE)
        GPK_LAUNCH("gpk_triangulate", (triangulate_rows_kernel<tri::TRI_G_LARGE, tri::TRI_SLICE_LARGE>), grid, dim3(256), 0, s, d, n, lists, tris, counts, status_dev);
    else
        GPK_LAUNCH("gpk_triangulate", (triangulate_rows_kernel<tri::TRI_G_SMALL, tri::TRI_SLICE_SMALL>), grid, dim3(256), 0, s, d, n, lists, tris, counts, status_dev);
    if (any_big) {
        const size_t lds = (size_t)tri::NODE_BYTES * tri::TRI_LDS_NODES;
        GPK_TRY(allow_lds(lds));
        int64_t blocks = total_share / (slice + 1);  // at most this many rows are above the slice
        if (blocks > n) blocks = n;
        GPK_LAUNCH("gpk_triangulate_large", triangulate_list_kernel<false>, dim3((unsigned)blocks), dim3(BT), lds, s, d, (const int32_t*)lists.big,
                   (char*)nullptr, tris, counts, status_dev);
    }
    if (any_huge) {
        int64_t blocks = total_share / (tri::TRI_LDS_NODES + 1);
        if (blocks > n) blocks = n;
        GPK_LAUNCH("gpk_triangulate_huge", triangulate_list_kernel<true>, dim3((unsigned)blocks), dim3(BT), 0, s, d, (const int32_t*)lists.huge, node_scratch,
                   tris, counts, status_dev);
    }
    GPK_TRY(exclusive_scan_i32(counts, n, offsets_dev, nullptr, block_tot, s));
    unsigned long long total = 0;
    GPK_HIP(d2h_small(&total, block_tot + (n + 255) / 256, sizeof total, s));
    if (host_out) GPK_HIP(hipMemcpyAsync(out_tri_offsets, offsets_dev, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, s));
    if (out_status && host_out) GPK_HIP(hipMemcpyAsync(out_status, status_dev, (size_t)n, hipMemcpyDeviceToHost, s));
    GPK_HIP(sync_small(s));
    *n_triangles = (int64_t)total;
    if (!out_index) return GPK_OK;
    if ((int64_t)total > tri_capacity)
        return fail(GPK_ERR_CAPACITY, "triangulate: %lld triangles, capacity %lld", (long long)total, (long long)tri_capacity);
    if (total == 0) return GPK_OK;
    Scratch sc_index(workspace_aux(0));
    uint32_t* index_dev;
    sc_index.stage(index_dev, out_index, out_space, 3 * (size_t)total);
    GPK_TRY(sc_index.commit());
    GPK_LAUNCH("gpk_triangulate_gather", triangulate_gather_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, d, n, (const uint32_t*)tris,
               (const int32_t*)offsets_dev, index_dev);
    return sc_index.copy_back(s);
}
