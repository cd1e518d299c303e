// gpk_validity.hip — gpk_validity and gpk_is_simple over the device routines of gpk_validity.h.  Contract: include/geopolars_hip.h.
//
// Two launches a call.  The first gives G lanes to every row (G = val::validity_group_size: 4 or 16) and finishes the rows of at most
// VAL_BLOCK_COORDS coordinates; a larger row is put on a list.  The second has one work-group per listed row (a grid-stride loop over
// the list, whose length stays on the device): shape pass, strip lists in LDS, the pair tests strip by strip, then codes 5 - 8 on
// the first 16 lanes.  Scratch: the list and, for code 8, one int per ring of the column.
#include "gpk_device.h"
#include "gpk_validity.h"

namespace gpk {

namespace {

using val::NONE;

// ---- G lanes per row ----------------------------------------------------------------------------------------------------------------
template <int G, bool POLY>
__global__ __launch_bounds__(256) void validity_rows_kernel(DevGeo g, int64_t n, int32_t* __restrict__ parent, int32_t* __restrict__ big,
                                                            uint8_t* __restrict__ out_code, int32_t* __restrict__ out_where) {
    const val::GroupCtx<G> cx{(int)(threadIdx.x & (G - 1))};
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += groups) {
        int code = GPK_VALID, where = -1;
        if (!dev::valid_row(g.validity, i)) {
            code = POLY ? GPK_INVALID_NULL : 1;  // (a line: not simple)
        } else {
            const val::Row r = POLY ? val::polygon_row(g, i) : val::line_row(g, i);
            if (r.c1 - r.c0 > val::VAL_BLOCK_COORDS) {
                if (cx.lane == 0) big[1 + atomicAdd(big, 1)] = (int32_t)i;
                continue;
            }
            const val::Shape sh = val::row_shape(r, cx);
            code = val::early_code(sh, where);
            if (code == GPK_VALID) {
                val::Found f{NONE, NONE, 0};
                val::all_pairs(r, cx, f);
                f.self = cx.imin(f.self);
                f.cross = cx.imin(f.cross);
                f.touch = cx.ior(f.touch);
                code = val::pair_code(sh, f, where);
                if constexpr (POLY)
                    if (code == GPK_VALID) code = val::row_nesting<G>(g, r, i, f.touch != 0, parent, cx.lane, where);
            }
        }
        if (cx.lane == 0) {
            out_code[i] = POLY ? (uint8_t)code : (uint8_t)(code == GPK_VALID);
            if (POLY && out_where) out_where[i] = where;
        }
    }
}

// ---- a work-group per large row -----------------------------------------------------------------------------------------------------
struct Strips {
    bool by_x;
    double lo, inv;
    int k;
    __device__ __forceinline__ int of(double2 p) const {
        const int s = (int)(((by_x ? p.x : p.y) - lo) * inv);  // monotone in the coordinate: a shared point lies in a shared strip
        return s < 0 ? 0 : (s >= k ? k - 1 : s);
    }
};

template <bool POLY>
__global__ __launch_bounds__(val::VAL_BLOCK_THREADS) void validity_big_kernel(DevGeo g, int32_t* __restrict__ parent, const int32_t* __restrict__ big,
                                                                               uint8_t* __restrict__ out_code, int32_t* __restrict__ out_where) {
    __shared__ int start[val::VAL_STRIPS_MAX + 1];
    __shared__ int cursor[val::VAL_STRIPS_MAX];
    __shared__ int entry[val::VAL_ENTRIES];
    __shared__ int red[8];
    __shared__ double wbox[val::VAL_BLOCK_THREADS / 64][4];
    const int tid = threadIdx.x;
    const val::BlockCtx cx{tid, &red[0]};
    const int n_big = big[0];
    for (int q = blockIdx.x; q < n_big; q += gridDim.x) {
        const int64_t i = big[1 + q];
        const val::Row r = POLY ? val::polygon_row(g, i) : val::line_row(g, i);
        int where = -1;
        const val::Shape sh = val::row_shape(r, cx);
        int code = val::early_code(sh, where);
        if (code == GPK_VALID) {
            val::Found f{NONE, NONE, 0};
            const int nseg = r.c1 - r.c0 - 1;
            // the row's box (finite coordinates) and the strips along its longer axis
            {
                double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
                for (int c = r.c0 + tid; c < r.c1; c += val::VAL_BLOCK_THREADS) {
                    const double2 p = r.xy[c];
                    mnx = fmin(mnx, p.x); mny = fmin(mny, p.y); mxx = fmax(mxx, p.x); mxy = fmax(mxy, p.y);
                }
                mnx = dev::wave_min(mnx); mny = dev::wave_min(mny); mxx = dev::wave_max(mxx); mxy = dev::wave_max(mxy);
                if ((tid & 63) == 0) {
                    double* w = wbox[tid >> 6];
                    w[0] = mnx; w[1] = mny; w[2] = mxx; w[3] = mxy;
                }
            }
            __syncthreads();
            double box[4] = {wbox[0][0], wbox[0][1], wbox[0][2], wbox[0][3]};
            for (int w = 1; w < val::VAL_BLOCK_THREADS / 64; ++w) {
                box[0] = fmin(box[0], wbox[w][0]); box[1] = fmin(box[1], wbox[w][1]);
                box[2] = fmax(box[2], wbox[w][2]); box[3] = fmax(box[3], wbox[w][3]);
            }
            __syncthreads();
            Strips st;
            st.by_x = box[2] - box[0] >= box[3] - box[1];
            st.lo = st.by_x ? box[0] : box[1];
            const double ext = (st.by_x ? box[2] : box[3]) - st.lo;
            st.k = nseg / val::VAL_SEGS_PER_STRIP;
            st.k = st.k < 1 ? 1 : (st.k > val::VAL_STRIPS_MAX ? val::VAL_STRIPS_MAX : st.k);
            if (!(ext > 0.0) || !(ext < INFINITY)) st.k = 1;
            int total;
            for (;;) {  // count the entries; too many: wider strips
                st.inv = st.k > 1 ? (double)st.k / ext : 0.0;
                for (int s = tid; s <= st.k; s += val::VAL_BLOCK_THREADS) start[s] = 0;
                __syncthreads();
                for (int c = r.c0 + tid; c + 1 < r.c1; c += val::VAL_BLOCK_THREADS) {
                    const double2 a = r.xy[c], b = r.xy[c + 1];
                    if (cont::same_xy(a, b)) continue;
                    const int sa = st.of(a), sb = st.of(b);
                    for (int s = sa < sb ? sa : sb; s <= (sa < sb ? sb : sa); ++s) atomicAdd(&start[s + 1], 1);
                }
                __syncthreads();
                if (tid == 0) {
                    int run = 0;
                    for (int s = 1; s <= st.k; ++s) {
                        run += start[s];
                        start[s] = run;
                    }
                    red[1] = run;
                }
                __syncthreads();
                total = red[1];
                __syncthreads();
                if (total <= val::VAL_ENTRIES || st.k == 1) break;
                st.k >>= 1;
            }
            if (total > val::VAL_ENTRIES) {
                val::all_pairs(r, cx, f);  // (more segments than the lists hold)
            } else {
                for (int s = tid; s < st.k; s += val::VAL_BLOCK_THREADS) cursor[s] = start[s];
                __syncthreads();
                for (int c = r.c0 + tid; c + 1 < r.c1; c += val::VAL_BLOCK_THREADS) {
                    const double2 a = r.xy[c], b = r.xy[c + 1];
                    if (cont::same_xy(a, b)) continue;
                    const int sa = st.of(a), sb = st.of(b);
                    for (int s = sa < sb ? sa : sb; s <= (sa < sb ? sb : sa); ++s) entry[atomicAdd(&cursor[s], 1)] = c;
                }
                __syncthreads();
                // a wave per strip; the lanes take the m x m pairs of its list, each unordered pair once, in the first strip it shares
                const int wave = tid >> 6, wl = tid & 63;
                for (int s = wave; s < st.k; s += val::VAL_BLOCK_THREADS / 64) {
                    const int e0 = start[s], m = start[s + 1] - e0;
                    for (int k = wl; k < m * m; k += 64) {
                        int ci = entry[e0 + k / m], cj = entry[e0 + k % m];
                        if (ci >= cj) continue;
                        const double2 a = r.xy[ci], b = r.xy[ci + 1];
                        const int si_lo = min(st.of(a), st.of(b)), sj_lo = min(st.of(r.xy[cj]), st.of(r.xy[cj + 1]));
                        if (s != (si_lo > sj_lo ? si_lo : sj_lo)) continue;
                        const int si = seq_of(r.so, r.s0, r.s1, ci);
                        const int i0 = r.so[si], i1 = r.so[si + 1];
                        if (ci + 1 >= i1 || !val::live(r, si)) continue;
                        val::pair_test(r, si, i0, i1, ci, a, b, cj, f);
                    }
                }
            }
            f.self = cx.imin(f.self);
            f.cross = cx.imin(f.cross);
            f.touch = cx.ior(f.touch);
            code = val::pair_code(sh, f, where);
            if constexpr (POLY) {
                if (code == GPK_VALID) {
                    if (tid < 16) {
                        int w;
                        const int c = val::row_nesting<16>(g, r, i, f.touch != 0, parent, tid, w);
                        if (tid == 0) {
                            red[2] = c;
                            red[3] = w;
                        }
                    }
                    __syncthreads();
                    code = red[2];
                    where = red[3];
                    __syncthreads();
                }
            }
        }
        if (tid == 0) {
            out_code[i] = POLY ? (uint8_t)code : (uint8_t)(code == GPK_VALID);
            if (POLY && out_where) out_where[i] = where;
        }
    }
}

template <bool POLY>
int32_t run(const gpk_geoarray* a, uint8_t* out_code, int32_t* out_where, int32_t out_space, hipStream_t s) {
    const DevGeo& g = a->d;
    const int64_t n = g.n_geoms;
    if (n > (int64_t)INT32_MAX - 1) return fail(GPK_ERR_INVALID_ARGUMENT, "%s: more than 2^31 - 2 rows", POLY ? "validity" : "is_simple");
    const bool host_out = out_space != GPK_MEM_DEVICE;
    const bool want_where = POLY && out_where;
    const bool want_parent = POLY && g.n_rings > 1;  // (a column of one ring has no member of two)
    const size_t where_bytes = sizeof(int32_t) * (size_t)n;
    Scratch sc(workspace());
    int32_t *big, *parent, *where_dev;
    uint8_t* code_dev;
    sc.add(big, (size_t)(n + 1));
    sc.add_if(want_parent, parent, (size_t)g.n_rings);
    sc.stage(code_dev, out_code, out_space, (size_t)n);
    sc.stage(where_dev, want_where ? out_where : nullptr, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    GPK_HIP(hipMemsetAsync(big, 0, sizeof(int32_t), s));
    const int G = val::validity_group_size(g);
    const dim3 grid = group_grid(n, G);
    const char* name = POLY ? "gpk_validity" : "gpk_is_simple";
    if (G == val::VAL_G_SMALL)
        GPK_LAUNCH(name, (validity_rows_kernel<val::VAL_G_SMALL, POLY>), grid, dim3(256), 0, s, g, n, parent, big, code_dev, where_dev);
    else
        GPK_LAUNCH(name, (validity_rows_kernel<val::VAL_G_LARGE, POLY>), grid, dim3(256), 0, s, g, n, parent, big, code_dev, where_dev);
    if (g.n_coords > val::VAL_BLOCK_COORDS) {  // (else no row can be on the list)
        int64_t blocks = g.n_coords / val::VAL_BLOCK_COORDS;  // at most this many rows are large
        if (blocks > n) blocks = n;
        if (blocks > (int64_t)cu_count() * 8) blocks = (int64_t)cu_count() * 8;
        GPK_LAUNCH(POLY ? "gpk_validity_large" : "gpk_is_simple_large", validity_big_kernel<POLY>, dim3((unsigned)blocks), dim3(val::VAL_BLOCK_THREADS), 0,
                   s, g, parent, big, code_dev, where_dev);
    }
    if (want_where && host_out) GPK_HIP(hipMemcpyAsync(out_where, where_dev, where_bytes, hipMemcpyDeviceToHost, s));
    return copy_out(out_code, out_space, code_dev, (size_t)n, s);
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_validity(const gpk_geoarray* a, uint8_t* out_code, int32_t* out_where, int32_t out_space, void* stream) {
    if (!a || !out_code) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_polygonal(a->d.type)) return fail(GPK_ERR_MISMATCHED_GEOMETRY, "validity: POLYGON | MULTIPOLYGON (found type %d)", a->d.type);
    GPK_TRY(require_device());
    if (a->d.n_geoms == 0) return GPK_OK;
    return run<true>(a, out_code, out_where, out_space, (hipStream_t)stream);
}

extern "C" int32_t gpk_is_simple(const gpk_geoarray* a, uint8_t* out, int32_t out_space, void* stream) {
    if (!a || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    if (a->d.type != GPK_GEOM_LINESTRING && a->d.type != GPK_GEOM_MULTILINESTRING)
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "is_simple: LINESTRING | MULTILINESTRING (found type %d)", a->d.type);
    GPK_TRY(require_device());
    if (a->d.n_geoms == 0) return GPK_OK;
    return run<false>(a, out, nullptr, out_space, (hipStream_t)stream);
}
