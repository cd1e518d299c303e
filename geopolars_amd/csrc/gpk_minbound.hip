// gpk_minbound.hip — gpk_minimum_rotated_rectangle and gpk_minimum_bounding_circle over the rules of gpk_minbound.h.
// Contract: include/geopolars_hip.h.  Both are functions of the row's convex hull alone: the hull stage of gpk_hull.hip (gpk_hull.h)
// leaves every row's exact hull in workspace scratch, then one launch gives MBG_G lanes to every row — one group per row on an uncapped
// grid, no loop over rows — and finishes the rows whose hull has at most MBG_SMALL_HULL vertices with the hull in LDS; the others are
// listed and taken by a work-group each (a constant grid of at most MBG_BIG_BLOCKS work-groups striding over the list).
//   rectangle, lane group   edges strided over the lanes, every lane scans all hull vertices for its edges (h * h / MBG_G vertex visits a
//                           row), then the group reduces to the best edge with the cross-multiplied comparison.
//   rectangle, work-group   rotating calipers (mb::caliper_edge): every thread takes a contiguous chunk of edges, walks the three support
//                           vertices of its first edge out from the edge's end and advances them monotonically from edge to edge,
//                           each advance decided from the hull edge itself and bounded by h: O(h) a thread, a 100k-vertex hull is
//                           legal input.
//   circle                  the farthest-point iteration; the search for the farthest vertex is the reduction, the O(1) update runs
//                           redundantly on every lane.  At most MBG_CIRCLE_ITERS iterations.
// A row's input coordinates are tested for finiteness by the same lanes first (the hull of a row with a NaN is never read).
#include "gpk_device.h"
#include "gpk_hull.h"
#include "gpk_minbound.h"

namespace gpk {

namespace {

constexpr int OP_RECT = 0, OP_CIRCLE = 1;
constexpr int G = mb::MBG_G;
constexpr int BT = mb::MBG_BIG_THREADS;

__device__ __forceinline__ bool finite2(double2 p) { return fabs(p.x) < INFINITY && fabs(p.y) < INFINITY; }  // (false for NaN)

struct Out {
    double2* rect;     // n * 5
    double2* centre;   // n, may be nullptr
    double* radius;    // n
    uint8_t* valid;    // n, may be nullptr
};

template <int OP>
__device__ __forceinline__ void write_none(const Out& o, int64_t g) {
    if (OP == OP_RECT) {
        for (int k = 0; k < 5; ++k) o.rect[5 * g + k] = make_double2(NAN, NAN);
    } else {
        if (o.centre) o.centre[g] = make_double2(NAN, NAN);
        o.radius[g] = NAN;
    }
    if (o.valid) o.valid[g] = 0;
}
__device__ __forceinline__ void write_rect(const Out& o, int64_t g, const mb::Rect& c) {
    double2* __restrict__ r = o.rect + 5 * g;
    r[0] = make_double2(c.x0, c.y0);
    r[1] = make_double2(c.x1, c.y1);
    r[2] = make_double2(c.x2, c.y2);
    r[3] = make_double2(c.x3, c.y3);
    r[4] = make_double2(c.x0, c.y0);
    if (o.valid) o.valid[g] = 1;
}
__device__ __forceinline__ void write_circle(const Out& o, int64_t g, double cx, double cy, double r) {
    if (o.centre) o.centre[g] = make_double2(cx, cy);
    o.radius[g] = r;
    if (o.valid) o.valid[g] = 1;
}
// the rows the hull stage settles by itself: one distinct point (closed ring p p), all collinear (p q p)
template <int OP>
__device__ __forceinline__ void write_flat(const Out& o, int64_t g, double2 p, double2 q) {
    if (OP == OP_RECT) {
        write_rect(o, g, mb::rect_flat(p.x, p.y, q.x, q.y));
    } else {
        const mb::Circle k = mb::circle_start(q.x - p.x, q.y - p.y, 1);
        write_circle(o, g, p.x + k.cx, p.y + k.cy, sqrt(k.r2));
    }
}

// ---- reductions over the MBG_G lanes of a row -------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ mb::Edge dpp_edge(const mb::Edge& e) {
    return mb::Edge{dev::dpp_mov<CTRL>(e.A), dev::dpp_mov<CTRL>(e.L2), dev::dpp_mov<CTRL>(e.smin), dev::dpp_mov<CTRL>(e.smax), dev::dpp_mov<CTRL>(e.tmax),
                    dev::dpp_mov<CTRL>(e.i)};
}
__device__ __forceinline__ mb::Edge group_best_edge(mb::Edge e) {  // (edge_pick is symmetric: the same bits on every lane)
    e = mb::edge_pick(e, dpp_edge<0xB1>(e));
    e = mb::edge_pick(e, dpp_edge<0x4E>(e));
    e = mb::edge_pick(e, dpp_edge<0x141>(e));
    e = mb::edge_pick(e, dpp_edge<0x140>(e));
    return e;
}
__device__ __forceinline__ mb::Far group_far(const mb::Far& f) {
    const double d = dev::group_max<G>(f.d2);
    const int i = dev::group_allreduce<G>(f.d2 == d ? f.index : mb::NO_EDGE, [](int a, int b) { return a < b ? a : b; });
    return mb::Far{d, i};
}
__device__ __forceinline__ void group_lds_sync() {  // the lanes of a group sit in one wave: a compiler-level fence orders the LDS traffic
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One group per row, no loop over rows.  big[0] counts the listed rows, big[1 ..] are their ids.
template <int OP>
__global__ __launch_bounds__(256) void minbound_rows_kernel(DevGeo a, int64_t n, const double2* __restrict__ stack, const int32_t* __restrict__ sizes,
                                                            const int32_t* __restrict__ n_pts, int32_t* __restrict__ big, Out o) {
    // one slot of padding a slice: the four groups of a wave read the same index of four slices at once
    __shared__ double2 lds[256 / G][mb::MBG_SMALL_HULL + 1];
    const int lane = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const int64_t g = (int64_t)blockIdx.x * (256 / G) + grp;
    if (g >= n) return;  // (group-uniform, as is every branch below)
    int c0, c1;
    geom_coord_range(a, g, c0, c1);
    bool ok = n_pts[g] > 0;
    if (ok) {
        int bad = 0;
        for (int c = c0 + lane; c < c1; c += G) bad |= finite2(a.xy[c]) ? 0 : 1;
        ok = dev::group_or<G>(bad) == 0;
    }
    if (!ok) {
        if (lane == 0) write_none<OP>(o, g);
        return;
    }
    const double2* __restrict__ hull = hull_slice(const_cast<double2*>(stack), c0, g);
    const int h = sizes[g] - 1;  // the ring without its closing vertex
    if (h < 1) {  // (no hull: the stage gives every row with a point one)
        if (lane == 0) write_none<OP>(o, g);
        return;
    }
    if (h <= 2) {
        if (lane == 0) write_flat<OP>(o, g, hull[0], hull[h - 1]);
        return;
    }
    if (h > mb::MBG_SMALL_HULL) {
        if (lane == 0) big[1 + atomicAdd(big, 1)] = (int32_t)g;
        return;
    }
    double2* __restrict__ v = lds[grp];
    for (int k = lane; k < h; k += G) v[k] = hull[k];
    group_lds_sync();
    if (OP == OP_RECT) {
        mb::Edge mine = mb::no_edge();
        for (int i = lane; i < h; i += G) {
            const double2 p = v[i], q = v[i + 1 == h ? 0 : i + 1];
            const double dx = q.x - p.x, dy = q.y - p.y;
            mb::Extent e = mb::extent_start();
            for (int k = 0; k < h; ++k) mb::extent_see(e, p.x, p.y, dx, dy, v[k].x, v[k].y);
            const mb::Edge cand = mb::edge_of(i, dx, dy, e);
            if (mb::edge_better(cand, mine)) mine = cand;
        }
        const mb::Edge best = group_best_edge(mine);
        const double2 p = v[best.i], q = v[best.i + 1 == h ? 0 : best.i + 1];  // (h >= 3: every group has an edge)
        if (lane == 0) write_rect(o, g, mb::rect_corners(p.x, p.y, q.x - p.x, q.y - p.y, best));
    } else {
        const double2 v0 = v[0];
        mb::Far f = mb::no_far();
        for (int k = lane; k < h; k += G) mb::far_see(f, mb::dist2(v[k].x - v0.x, v[k].y - v0.y, 0.0, 0.0), k);
        f = group_far(f);
        mb::Circle cir = mb::circle_start(v[f.index].x - v0.x, v[f.index].y - v0.y, f.index);
        bool done = false;
        for (int it = 0; it < MBG_CIRCLE_ITERS; ++it) {
            f = mb::no_far();
            for (int k = lane; k < h; k += G) mb::far_see(f, mb::dist2(v[k].x - v0.x, v[k].y - v0.y, cir.cx, cir.cy), k);
            f = group_far(f);
            if (mb::circle_done(cir, f)) {
                done = true;
                break;
            }
            cir = mb::circle_step(cir, v[f.index].x - v0.x, v[f.index].y - v0.y, f.index);
        }
        if (!done) {  // out of iterations: the current centre, grown to the farthest vertex
            f = mb::no_far();
            for (int k = lane; k < h; k += G) mb::far_see(f, mb::dist2(v[k].x - v0.x, v[k].y - v0.y, cir.cx, cir.cy), k);
            cir.r2 = group_far(f).d2;
        }
        if (lane == 0) write_circle(o, g, v0.x + cir.cx, v0.y + cir.cy, sqrt(cir.r2));
    }
}

// ---- a work-group per listed row ----------------------------------------------------------------------------------------------------
struct BlockRed {
    int tid;
    double* dslot;       // LDS, BT / 64 doubles
    int* islot;          // LDS, one int
    mb::Edge* eslot;     // LDS, BT / 64 edges
    __device__ __forceinline__ mb::Far far(const mb::Far& f) const {
        const double w = dev::wave_max(f.d2);
        if ((tid & 63) == 0) dslot[tid >> 6] = w;
        if (tid == 0) *islot = mb::NO_EDGE;
        __syncthreads();
        double d = dslot[0];
        for (int k = 1; k < BT / 64; ++k) d = fmax(d, dslot[k]);
        if (f.d2 == d && f.index != mb::NO_EDGE) atomicMin(islot, f.index);
        __syncthreads();
        const int i = *islot;
        __syncthreads();
        return mb::Far{d, i};
    }
    __device__ __forceinline__ mb::Edge best_edge(mb::Edge e) const {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const mb::Edge p{__shfl_xor(e.A, off, 64), __shfl_xor(e.L2, off, 64), __shfl_xor(e.smin, off, 64), __shfl_xor(e.smax, off, 64),
                             __shfl_xor(e.tmax, off, 64), __shfl_xor(e.i, off, 64)};
            e = mb::edge_pick(e, p);
        }
        if ((tid & 63) == 0) {  // (field by field: a struct copy would go through scratch memory)
            mb::Edge& w = eslot[tid >> 6];
            w.A = e.A, w.L2 = e.L2, w.smin = e.smin, w.smax = e.smax, w.tmax = e.tmax, w.i = e.i;
        }
        __syncthreads();
        auto slot = [&](int k) { return mb::Edge{eslot[k].A, eslot[k].L2, eslot[k].smin, eslot[k].smax, eslot[k].tmax, eslot[k].i}; };
        mb::Edge r = slot(0);
#pragma unroll
        for (int k = 1; k < BT / 64; ++k) r = mb::edge_pick(r, slot(k));
        __syncthreads();
        return r;
    }
};

template <int OP>
__global__ __launch_bounds__(BT) void minbound_big_kernel(DevGeo a, const double2* __restrict__ stack, const int32_t* __restrict__ sizes,
                                                          const int32_t* __restrict__ big, Out o) {
    __shared__ double2 lds[mb::MBG_LDS_HULL];
    __shared__ double dslot[BT / 64];
    __shared__ int islot;
    __shared__ mb::Edge eslot[BT / 64];
    const int tid = threadIdx.x;
    const BlockRed red{tid, dslot, &islot, eslot};
    const int n_big = big[0];
    for (int b = blockIdx.x; b < n_big; b += gridDim.x) {
        const int64_t g = big[1 + b];
        int c0, c1;
        geom_coord_range(a, g, c0, c1);
        const double2* __restrict__ hull = hull_slice(const_cast<double2*>(stack), c0, g);
        const int h = sizes[g] - 1;
        const bool in_lds = h <= mb::MBG_LDS_HULL;  // block-uniform
        if (in_lds)
            for (int k = tid; k < h; k += BT) lds[k] = hull[k];
        __syncthreads();
        auto ld = [&](int k) -> double2 { return in_lds ? lds[k] : hull[k]; };
        auto nx = [&](int k) -> int { return k + 1 == h ? 0 : k + 1; };
        if (OP == OP_RECT) {
            const int per = (h + BT - 1) / BT;
            const int e0 = tid * per < h ? tid * per : h, e1 = e0 + per < h ? e0 + per : h;
            mb::Edge mine = mb::no_edge();
            mb::Calipers cal{0, 0, 0};
            for (int i = e0; i < e1; ++i) {
                const mb::Edge cand = mb::caliper_edge(ld, h, i, i == e0, cal);
                if (mb::edge_better(cand, mine)) mine = cand;
            }
            const mb::Edge best = red.best_edge(mine);
            if (tid == 0) {
                const double2 p = ld(best.i), q = ld(nx(best.i));
                write_rect(o, g, mb::rect_corners(p.x, p.y, q.x - p.x, q.y - p.y, best));
            }
        } else {
            const double2 v0 = ld(0);
            auto farthest = [&](double cx, double cy) {
                mb::Far f = mb::no_far();
                for (int k = tid; k < h; k += BT) {
                    const double2 w = ld(k);
                    mb::far_see(f, mb::dist2(w.x - v0.x, w.y - v0.y, cx, cy), k);
                }
                return red.far(f);
            };
            auto local = [&](int k, double& x, double& y) {
                const double2 w = ld(k);
                x = w.x - v0.x, y = w.y - v0.y;
            };
            mb::Far f = farthest(0.0, 0.0);
            double qx, qy;
            local(f.index, qx, qy);
            mb::Circle cir = mb::circle_start(qx, qy, f.index);
            bool done = false;
            for (int it = 0; it < MBG_CIRCLE_ITERS; ++it) {
                f = farthest(cir.cx, cir.cy);
                if (mb::circle_done(cir, f)) {
                    done = true;
                    break;
                }
                local(f.index, qx, qy);
                cir = mb::circle_step(cir, qx, qy, f.index);
            }
            if (!done) cir.r2 = farthest(cir.cx, cir.cy).d2;
            if (tid == 0) write_circle(o, g, v0.x + cir.cx, v0.y + cir.cy, sqrt(cir.r2));
        }
        __syncthreads();  // the LDS hull is rewritten by the work-group's next row
    }
}

// POINT columns: a finite point is its own hull
template <int OP>
__global__ void minbound_point_kernel(DevGeo a, int64_t n, Out o) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const double2 p = a.xy[g];
    if (dev::valid_row(a.validity, g) && finite2(p))
        write_flat<OP>(o, g, p, p);
    else
        write_none<OP>(o, g);
}

template <int OP>
int32_t run(const gpk_geoarray* a, double* out_rect, double* out_centre, double* out_radius, uint8_t* out_valid, int32_t out_space, hipStream_t s) {
    const DevGeo& d = a->d;
    const int64_t n = d.n_geoms, nc = d.n_coords;
    if (n == 0) return GPK_OK;
    if (n > (int64_t)INT32_MAX - 1) return fail(GPK_ERR_INVALID_ARGUMENT, "minimum bounding shapes: more than 2^31 - 2 rows");
    const bool point = d.type == GPK_GEOM_POINT;
    const size_t rect_bytes = sizeof(double2) * 5 * (size_t)n, xy_bytes = sizeof(double2) * (size_t)n, r_bytes = sizeof(double) * (size_t)n;
    Scratch sc(workspace());
    HullStage hs{};
    if (!point) hull_stage_plan(sc, n, nc, &hs);
    int32_t* big;
    sc.add(big, (size_t)(n + 1));
    Out o{nullptr, nullptr, nullptr, nullptr};
    if (OP == OP_RECT) {
        sc.stage(o.rect, (double2*)out_rect, out_space, 5 * (size_t)n);
    } else {
        sc.stage(o.centre, (double2*)out_centre, out_space, (size_t)n);
        sc.stage(o.radius, out_radius, out_space, (size_t)n);
    }
    sc.stage(o.valid, out_valid, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    if (!point) GPK_TRY(hull_stage(a, hs, s));
    const char* name = OP == OP_RECT ? "gpk_minimum_rotated_rectangle" : "gpk_minimum_bounding_circle";
    const char* name_large = OP == OP_RECT ? "gpk_minimum_rotated_rectangle_large" : "gpk_minimum_bounding_circle_large";
    if (point) {
        GPK_LAUNCH(name, minbound_point_kernel<OP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, n, o);
    } else {
        GPK_HIP(hipMemsetAsync(big, 0, sizeof(int32_t), s));
        const int64_t per_block = 256 / G;
        GPK_LAUNCH(name, minbound_rows_kernel<OP>, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, s, d, n, (const double2*)hs.stack,
                   (const int32_t*)hs.sizes, (const int32_t*)hs.n_pts, big, o);
        if (nc > mb::MBG_SMALL_HULL) {  // (else no row can be on the list)
            const int64_t blocks = n < mb::MBG_BIG_BLOCKS ? n : mb::MBG_BIG_BLOCKS;
            GPK_LAUNCH(name_large, minbound_big_kernel<OP>, dim3((unsigned)blocks), dim3(BT), 0, s, d, (const double2*)hs.stack, (const int32_t*)hs.sizes,
                       (const int32_t*)big, o);
        }
    }
    if (out_valid) GPK_TRY(copy_out(out_valid, out_space, o.valid, (size_t)n, s));
    if (OP == OP_RECT) return copy_out(out_rect, out_space, o.rect, rect_bytes, s);
    if (out_centre) GPK_TRY(copy_out(out_centre, out_space, o.centre, xy_bytes, s));
    return copy_out(out_radius, out_space, o.radius, r_bytes, s);
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_minimum_rotated_rectangle(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, int32_t out_space, void* stream) {
    if (!a || !out_xy) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    GPK_TRY(require_device());
    return run<OP_RECT>(a, out_xy, nullptr, nullptr, out_valid, out_space, (hipStream_t)stream);
}

extern "C" int32_t gpk_minimum_bounding_circle(const gpk_geoarray* a, double* out_center_xy, double* out_radius, uint8_t* out_valid, int32_t out_space,
                                               void* stream) {
    if (!a || !out_radius) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    GPK_TRY(require_device());
    return run<OP_CIRCLE>(a, nullptr, out_center_xy, out_radius, out_valid, out_space, (hipStream_t)stream);
}
