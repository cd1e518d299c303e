// gpk_nearest.hip — nearest-neighbour join (GeoPandas sjoin_nearest): for every left POINT the right rows at the row's
// minimum Euclidean distance, ties included.  Contract: include/geopolars_hip.h (gpk_nearest_join).
//
// Search.  The right side's index is the uniform bbox grid of gpk_index.h (cell -> ids of the geometries whose closed bbox
// meets the cell).  A query starts in its own cell — the point clamped onto the grid, so a point outside the extent starts
// in a border cell and never walks the empty gap — and grows a visited RECTANGLE of cells one column or row at a time.
// Each step takes the side whose unvisited part (a rectangle of the extent: every cell beyond that side) is nearest to the
// point, so a point far to the left of a small extent visits the left border column first and moves right only as far as
// the distances ask for.  The walk stops when the nearest unvisited part is farther than the current best distance:
// strictly farther, so that a geometry exactly as far as the best one (a tie) is still reached.  `max_distance` is the
// starting bound.  A cell farther than the bound is skipped without reading its directory entries.
//
// Pruning.  A candidate whose bbox is farther than the bound is skipped before any of its coordinates is read.  Every
// bound is lowered by 64 ulps of the coordinates' magnitude (NearGrid::scale plus the point's): the cell borders come from
// the rounded cell function and the distances from rounded arithmetic, and a candidate skipped by a bound must be one whose
// computed distance cannot reach the best.  The margin only ever costs a few extra exact evaluations.
//
// Dedupe.  A geometry whose bbox spans several cells is listed in each of them.  It is evaluated only in the cell that holds
// the query point clamped onto its bbox (the nearest point of the bbox, which lies in one of the geometry's cells under the
// same monotone cell function the directory was built with) — once per query, and in the cell nearest to the query.
//
// Distances.  point_geom_distance<G, KIND> of gpk_distance.h with G = distance_group_size(right): the function, the group
// size and the lane order of gpk_distance_rowwise's per-row kernel, so a returned distance is the very double that
// gpk_distance_rowwise(left, right, b_rows) returns for the pair there.  (Its grouped schedule — LINESTRING right sides with
// eight or more rows per target on average — evaluates linestrings with a different instruction sequence and agrees to its
// 1e-9 contract, the zero / non-zero outcome exactly.)  Ties are equality of those doubles.
//
// Lanes.  G lanes per query walk the same cells and candidates (the loop is uniform across the group): the lanes test a
// cell's entries G at a time (id, bbox, dedupe, bbox bound), the survivors are taken one after the other by the whole group,
// whose lanes walk the candidate's segments strided and reduce with gmin_frac<G>.
//
// Ties without a limit.  Pass 1 (nearest_best_kernel) finds each row's minimum, the number of right rows at it and the
// smallest such row; a scan of the counts gives each row its slice of the output; pass 2 (nearest_emit_kernel) writes rows
// with one match straight from pass 1 and re-walks the rows with ties, bounded by the known minimum, writing every right row
// at it and sorting the slice by right id.  The output is sorted by (l, r).
#include <cfloat>

#include "gpk_device.h"
#include "gpk_distance.h"
#include "gpk_candjoin.h"
#include "gpk_index.h"
#include "gpk_scan.h"

namespace gpk {

// The directory's cell geometry as the walk needs it.  An axis of zero extent (all boxes on one line, or an index of empty
// rows only) has inv_w / inv_h = 0: the cell function sends everything to column / row 0, so that axis has one usable
// column / row of width 0.
struct NearGrid {
    double x0, y0, inv_w, inv_h;  // the directory's own parameters (the cell function)
    double cw, ch;                // cell width / height (0 on a degenerate axis)
    double scale;                 // |x0| + |y0| + extent width + extent height: the magnitude the bound margins scale with
    int32_t gx, gy;               // directory dimensions (cell id = cy * gx + cx)
    int32_t ex, ey;               // usable columns / rows
};

// What the kernels read of the left points and of the directory (the rest of DevGeo / IndexView stays out of the kernel arguments:
// every uniform value is a scalar register, and the walk keeps many of them live)
struct NearPts {
    const double2* xy;
    const uint8_t* validity;
    int64_t n;
};
struct NearDir {
    const double4* bbox;
    const int32_t* cell_off;
    const int32_t* items;
};

namespace {

__device__ __forceinline__ double rect_distance(double px, double py, double ax, double bx, double ay, double by) {
    const double dx = fmax(fmax(ax - px, px - bx), 0.0), dy = fmax(fmax(ay - py, py - by), 0.0);
    return sqrt(dx * dx + dy * dy);
}

// Visits, for one query, every right row that can lie within `bound` (see the header comment), calling on_hit(j, d) with the
// row and its distance, uniformly across the G lanes of the group.  on_hit may lower `bound`.
template <int G, int KIND, class F>
__device__ __forceinline__ void nearest_walk(const DevGeo& right, const NearDir& ix, const NearGrid& grid, double px, double py, int lane,
                                             int gbase, double& bound, F&& on_hit) {
    // The grid's doubles are uniform, but kept in vector registers: as scalars they, the directory's and the right side's pointers
    // and the distance code's own uniform values outgrow the scalar register file and spill
    NearGrid g = grid;
    asm volatile("" : "+v"(g.x0), "+v"(g.y0), "+v"(g.inv_w), "+v"(g.inv_h), "+v"(g.cw), "+v"(g.ch));
    const double m = 64.0 * DBL_EPSILON * (g.scale + fabs(px) + fabs(py));
    auto visit = [&](int cx, int cy) {
        const double ax = g.x0 + cx * g.cw, ay = g.y0 + cy * g.ch;
        if (rect_distance(px, py, ax, ax + g.cw, ay, ay + g.ch) - m > bound) return;
        const int c = cy * g.gx + cx;
        const int k0 = ix.cell_off[c], k1 = ix.cell_off[c + 1];
        for (int kb = k0; kb < k1; kb += G) {  // (group-uniform trip count)
            const int k = kb + lane;
            bool keep = false;
            int j = 0;
            double lb = 0.0;
            if (k < k1) {
                j = ix.items[k];
                const double4 b = ix.bbox[j];
                const double rx = fmin(fmax(px, b.x), b.z), ry = fmin(fmax(py, b.y), b.w);  // the point clamped onto the bbox
                if (dev::cell_of(rx, g.x0, g.inv_w, g.gx) == cx && dev::cell_of(ry, g.y0, g.inv_h, g.gy) == cy &&
                    dev::valid_row(right.validity, j)) {
                    const double dx = px - rx, dy = py - ry;
                    lb = sqrt(dx * dx + dy * dy);
                    keep = !(lb - m > bound);
                }
            }
            unsigned long long todo;
            if (G == 1)
                todo = keep ? 1ull : 0ull;
            else
                todo = (__ballot(keep) >> gbase) & (G == 64 ? ~0ull : ((1ull << G) - 1ull));
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const int jj = G == 1 ? j : __shfl(j, gbase + src, 64);
                const double lbj = G == 1 ? lb : __shfl(lb, gbase + src, 64);
                if (lbj - m > bound) continue;  // (the bound may have come down since the entries were tested)
                const double d = point_geom_distance<G, KIND>(right, jj, px, py, lane);
                on_hit(jj, d);
            }
        }
    };
    int ax0 = dev::cell_of(px, g.x0, g.inv_w, g.gx), ay0 = dev::cell_of(py, g.y0, g.inv_h, g.gy);
    if (ax0 >= g.ex) ax0 = g.ex - 1;
    if (ay0 >= g.ey) ay0 = g.ey - 1;
    int ax1 = ax0, ay1 = ay0;
    const double X0 = g.x0, X1 = g.x0 + g.ex * g.cw, Y0 = g.y0, Y1 = g.y0 + g.ey * g.ch;
    // the cells come one at a time from a cursor over the current line (the start cell, then one new column or row per step):
    // a single call site of visit() keeps one copy of the distance code in the kernel
    int cx = ax0, cy = ay0, sx = 0, sy = 0, left_in_line = 1;
    for (;;) {
        if (left_in_line == 0) {
            // distance to the unvisited cells beyond each side of the visited rectangle (all rows / columns of the extent)
            const double dl = ax0 > 0 ? rect_distance(px, py, X0, g.x0 + ax0 * g.cw, Y0, Y1) : INFINITY;
            const double dr = ax1 < g.ex - 1 ? rect_distance(px, py, g.x0 + (ax1 + 1) * g.cw, X1, Y0, Y1) : INFINITY;
            const double db = ay0 > 0 ? rect_distance(px, py, X0, X1, Y0, g.y0 + ay0 * g.ch) : INFINITY;
            const double dt = ay1 < g.ey - 1 ? rect_distance(px, py, X0, X1, g.y0 + (ay1 + 1) * g.ch, Y1) : INFINITY;
            int side = 0;
            double lo = dl;
            if (dr < lo) lo = dr, side = 1;
            if (db < lo) lo = db, side = 2;
            if (dt < lo) lo = dt, side = 3;
            if (lo == INFINITY || lo - m > bound) break;
            if (side < 2) {  // a new column, bottom to top
                cx = side == 0 ? --ax0 : ++ax1;
                cy = ay0;
                sx = 0;
                sy = 1;
                left_in_line = ay1 - ay0 + 1;
            } else {  // a new row, left to right
                cy = side == 2 ? --ay0 : ++ay1;
                cx = ax0;
                sx = 1;
                sy = 0;
                left_in_line = ax1 - ax0 + 1;
            }
        }
        visit(cx, cy);
        cx += sx;
        cy += sy;
        --left_in_line;
    }
}

__device__ __forceinline__ bool query_ok(const NearPts& pts, int64_t i, double2& p) {
    if (!dev::valid_row(pts.validity, i)) return false;
    p = pts.xy[i];
    return !isnan(p.x) && !isnan(p.y);
}

// Pass 1: per left row the minimum distance within max_d, how many right rows are at it, and the smallest of them.
template <int G, int KIND>
__global__ __launch_bounds__(256) void nearest_best_kernel(NearPts pts, DevGeo right, NearDir ix, NearGrid g, double max_d,
                                                           double* __restrict__ best_d, uint32_t* __restrict__ best_r, int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & (G - 1), gbase = (int)(threadIdx.x & 63) & ~(G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < pts.n; i += groups) {
        double best = INFINITY;
        uint32_t r = 0xFFFFFFFFu;
        int c = 0;
        double2 p;
        if (query_ok(pts, i, p)) {
            double bound = max_d;
            nearest_walk<G, KIND>(right, ix, g, p.x, p.y, lane, gbase, bound, [&](int j, double d) {
                if (!(d <= max_d)) return;
                if (d < best) {
                    best = d;
                    r = (uint32_t)j;
                    c = 1;
                    bound = d;
                } else if (d == best) {
                    ++c;
                    r = (uint32_t)j < r ? (uint32_t)j : r;
                }
            });
        }
        if (lane == 0) {
            best_d[i] = best;
            best_r[i] = r;
            cnt[i] = c;
        }
    }
}

// Pass 2: each row's slice [off[i], off[i] + cnt[i]) of the output.  Rows with ties walk again with their minimum as the bound.
template <int G, int KIND>
__global__ __launch_bounds__(256) void nearest_emit_kernel(NearPts pts, DevGeo right, NearDir ix, NearGrid g, const double* __restrict__ best_d,
                                                           const uint32_t* __restrict__ best_r, const int32_t* __restrict__ cnt,
                                                           const int32_t* __restrict__ off, uint32_t left_row_base, uint32_t* __restrict__ pairs,
                                                           double* __restrict__ dist) {
    const int lane = threadIdx.x & (G - 1), gbase = (int)(threadIdx.x & 63) & ~(G - 1);
    const int64_t groups = (int64_t)gridDim.x * (256 / G);
    for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < pts.n; i += groups) {
        const int c = cnt[i];
        if (c == 0) continue;
        const int64_t o = off[i];
        const double best = best_d[i];
        const uint32_t l = left_row_base + (uint32_t)i;
        if (c == 1) {
            if (lane == 0) {
                pairs[2 * o] = l;
                pairs[2 * o + 1] = best_r[i];
                if (dist) dist[o] = best;
            }
            continue;
        }
        double2 p = pts.xy[i];
        double bound = best;
        int t = 0;
        nearest_walk<G, KIND>(right, ix, g, p.x, p.y, lane, gbase, bound, [&](int j, double d) {
            if (d == best && t < c) {
                if (lane == 0) pairs[2 * (o + t) + 1] = (uint32_t)j;
                ++t;
            }
        });
        if (lane == 0) {
            // the slice in right-id order (shell sort: ties are few, but nothing limits them)
            uint32_t* rs = pairs + 2 * o + 1;
            int gap = 1;
            while (gap < t / 3) gap = 3 * gap + 1;
            for (; gap > 0; gap /= 3)
                for (int a = gap; a < t; ++a) {
                    const uint32_t key = rs[2 * a];
                    int b = a;
                    while (b >= gap && rs[2 * (b - gap)] > key) {
                        rs[2 * b] = rs[2 * (b - gap)];
                        b -= gap;
                    }
                    rs[2 * b] = key;
                }
            for (int a = 0; a < t; ++a) {
                pairs[2 * (o + a)] = l;
                if (dist) dist[o + a] = best;
            }
        }
    }
}

}  // namespace

static NearGrid near_grid_of(const gpk_index* ix) {
    const GridParams& h = ix->host_grid;
    NearGrid g;
    g.x0 = h.x0;
    g.y0 = h.y0;
    g.inv_w = h.inv_w;
    g.inv_h = h.inv_h;
    g.gx = h.gx;
    g.gy = h.gy;
    g.cw = h.inv_w > 0.0 ? 1.0 / h.inv_w : 0.0;
    g.ch = h.inv_h > 0.0 ? 1.0 / h.inv_h : 0.0;
    g.ex = h.inv_w > 0.0 ? h.gx : 1;
    g.ey = h.inv_h > 0.0 ? h.gy : 1;
    g.scale = fabs(g.x0) + fabs(g.y0) + g.ex * g.cw + g.ey * g.ch;
    return g;
}

template <int KIND>
static int32_t launch_best(int G, const NearPts& pts, const DevGeo& right, const NearDir& ix, const NearGrid& g, double max_d, double* best_d,
                           uint32_t* best_r, int32_t* cnt, hipStream_t s) {
    const dim3 grid = group_grid(pts.n, G);
    if (G == 1)
        GPK_LAUNCH("gpk_nearest_best", (nearest_best_kernel<1, KIND>), grid, dim3(256), 0, s, pts, right, ix, g, max_d, best_d, best_r, cnt);
    else if (G == 8)
        GPK_LAUNCH("gpk_nearest_best", (nearest_best_kernel<8, KIND>), grid, dim3(256), 0, s, pts, right, ix, g, max_d, best_d, best_r, cnt);
    else
        GPK_LAUNCH("gpk_nearest_best", (nearest_best_kernel<32, KIND>), grid, dim3(256), 0, s, pts, right, ix, g, max_d, best_d, best_r, cnt);
    return GPK_OK;
}
template <int KIND>
static int32_t launch_emit(int G, const NearPts& pts, const DevGeo& right, const NearDir& ix, const NearGrid& g, const double* best_d,
                           const uint32_t* best_r, const int32_t* cnt, const int32_t* off, uint32_t base, uint32_t* pairs, double* dist, hipStream_t s) {
    const dim3 grid = group_grid(pts.n, G);
    if (G == 1)
        GPK_LAUNCH("gpk_nearest_emit", (nearest_emit_kernel<1, KIND>), grid, dim3(256), 0, s, pts, right, ix, g, best_d, best_r, cnt, off, base, pairs, dist);
    else if (G == 8)
        GPK_LAUNCH("gpk_nearest_emit", (nearest_emit_kernel<8, KIND>), grid, dim3(256), 0, s, pts, right, ix, g, best_d, best_r, cnt, off, base, pairs, dist);
    else
        GPK_LAUNCH("gpk_nearest_emit", (nearest_emit_kernel<32, KIND>), grid, dim3(256), 0, s, pts, right, ix, g, best_d, best_r, cnt, off, base, pairs, dist);
    return GPK_OK;
}

}  // namespace gpk

using namespace gpk;

extern "C" int32_t gpk_nearest_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double max_distance,
                                    uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist, int64_t pair_capacity,
                                    int64_t* n_pairs, int32_t out_space, void* stream) {
    if (!left || !right || !n_pairs) return fail(GPK_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_pairs = 0;
    if (!(max_distance >= 0.0)) return fail(GPK_ERR_INVALID_ARGUMENT, "nearest_join: max_distance must be >= 0 (INFINITY: no limit), got %g", max_distance);
    if (pair_capacity < 0 || (pair_capacity > 0 && !out_pairs)) return fail(GPK_ERR_INVALID_ARGUMENT, "pair_capacity without out_pairs");
    if (left->d.type != GPK_GEOM_POINT) return fail(GPK_ERR_MISMATCHED_GEOMETRY, "nearest_join: the left side must be POINT (found type %d)", left->d.type);
    const int32_t rt = right->d.type;
    if (rt != GPK_GEOM_POINT && rt != GPK_GEOM_MULTIPOINT && rt != GPK_GEOM_LINESTRING && rt != GPK_GEOM_MULTILINESTRING && rt != GPK_GEOM_POLYGON &&
        rt != GPK_GEOM_MULTIPOLYGON)
        return fail(GPK_ERR_MISMATCHED_GEOMETRY, "nearest_join: unsupported right geometry type %d", rt);
    if (right_index) GPK_TRY(index_matches_with_grid(right_index, right, "nearest_join"));
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = left->d.n_geoms;
    if (n == 0) return GPK_OK;
    if (n > (int64_t)INT32_MAX) return fail(GPK_ERR_INVALID_ARGUMENT, "nearest_join: more than 2^31 - 1 left rows: shard the left side");

    gpk_index* tmp_index = nullptr;  // (built before the workspace is carved: the build uses the workspace itself)
    if (!right_index) {
        GPK_TRY(gpk_index_build_ex(right, GPK_INDEX_BBOX_GRID, nullptr, stream, &tmp_index));
        right_index = tmp_index;
    }
    auto done = [&](int32_t rc) {
        if (tmp_index) {
            (void)hipStreamSynchronize(s);
            gpk_index_free(tmp_index);
        }
        return rc;
    };
    const bool host_out = out_space != GPK_MEM_DEVICE;
    const bool want_pairs = pair_capacity > 0;
    const int G = distance_group_size(right->d);
    const NearGrid g = near_grid_of(right_index);
    const NearDir ix{right_index->v.bbox, right_index->v.cell_off, right_index->v.items};
    const NearPts pts{left->d.xy, left->d.validity, n};

    const int64_t nb = (n + 255) / 256;
    Scratch sc(workspace());
    double* best_d;
    uint32_t* best_r;
    int32_t *cnt, *off;
    unsigned long long* btot;
    sc.add(best_d, (size_t)n);
    sc.add_n((size_t)(n + 1), best_r, cnt, off);
    sc.add(btot, (size_t)(nb + 2));
    int32_t rc = sc.commit();
    if (rc != GPK_OK) return done(rc);

    auto pass1 = [&]() -> int32_t {
        switch (right->d.type) {
        case GPK_GEOM_POINT: return launch_best<GPK_GEOM_POINT>(1, pts, right->d, ix, g, max_distance, best_d, best_r, cnt, s);
        case GPK_GEOM_MULTIPOINT: return launch_best<GPK_GEOM_MULTIPOINT>(G, pts, right->d, ix, g, max_distance, best_d, best_r, cnt, s);
        case GPK_GEOM_LINESTRING: return launch_best<GPK_GEOM_LINESTRING>(G, pts, right->d, ix, g, max_distance, best_d, best_r, cnt, s);
        case GPK_GEOM_MULTILINESTRING: return launch_best<GPK_GEOM_MULTILINESTRING>(G, pts, right->d, ix, g, max_distance, best_d, best_r, cnt, s);
        case GPK_GEOM_POLYGON: return launch_best<GPK_GEOM_POLYGON>(G, pts, right->d, ix, g, max_distance, best_d, best_r, cnt, s);
        default: return launch_best<GPK_GEOM_MULTIPOLYGON>(G, pts, right->d, ix, g, max_distance, best_d, best_r, cnt, s);
        }
    };
    rc = pass1();
    if (rc != GPK_OK) return done(rc);
    rc = exclusive_scan_i32(cnt, n, off, nullptr, btot, s);
    if (rc != GPK_OK) return done(rc);
    unsigned long long total = 0;
    hipError_t e = d2h_small(&total, btot + nb, sizeof total, s);
    if (e == hipSuccess) e = sync_small(s);
    if (e != hipSuccess) return done(fail(GPK_ERR_DEVICE, "nearest_join: %s", hipGetErrorString(e)));
    if (total > (unsigned long long)INT32_MAX)
        return done(fail(GPK_ERR_CAPACITY, "nearest_join: %llu pairs exceed the i32 row offsets: shard the left side", total));
    *n_pairs = (int64_t)total;
    if (out_counts) {
        static_assert(sizeof(int32_t) == sizeof(uint32_t), "counts are copied bit for bit");
        rc = copy_out(out_counts, out_space, cnt, sizeof(uint32_t) * (size_t)n, s);
        if (rc == GPK_OK && !host_out && hipStreamSynchronize(s) != hipSuccess) rc = fail(GPK_ERR_DEVICE, "nearest_join: counts copy failed");
        if (rc != GPK_OK) return done(rc);
    }
    if (want_pairs && (int64_t)total > pair_capacity)
        return done(fail(GPK_ERR_CAPACITY, "nearest_join: %lld pairs but capacity %lld", (long long)total, (long long)pair_capacity));
    if (!want_pairs || total == 0) return done(GPK_OK);

    Scratch sc_out(workspace_aux(0));
    uint32_t* pairs_dev;
    double* dist_dev;
    sc_out.stage(pairs_dev, out_pairs, out_space, 2 * (size_t)total);
    sc_out.stage(dist_dev, out_dist, out_space, (size_t)total);
    rc = sc_out.commit();
    if (rc != GPK_OK) return done(rc);
    auto pass2 = [&]() -> int32_t {
        switch (right->d.type) {
        case GPK_GEOM_POINT:
            return launch_emit<GPK_GEOM_POINT>(1, pts, right->d, ix, g, best_d, best_r, cnt, off, left_row_base, pairs_dev, dist_dev, s);
        case GPK_GEOM_MULTIPOINT:
            return launch_emit<GPK_GEOM_MULTIPOINT>(G, pts, right->d, ix, g, best_d, best_r, cnt, off, left_row_base, pairs_dev, dist_dev, s);
        case GPK_GEOM_LINESTRING:
            return launch_emit<GPK_GEOM_LINESTRING>(G, pts, right->d, ix, g, best_d, best_r, cnt, off, left_row_base, pairs_dev, dist_dev, s);
        case GPK_GEOM_MULTILINESTRING:
            return launch_emit<GPK_GEOM_MULTILINESTRING>(G, pts, right->d, ix, g, best_d, best_r, cnt, off, left_row_base, pairs_dev, dist_dev, s);
        case GPK_GEOM_POLYGON:
            return launch_emit<GPK_GEOM_POLYGON>(G, pts, right->d, ix, g, best_d, best_r, cnt, off, left_row_base, pairs_dev, dist_dev, s);
        default:
            return launch_emit<GPK_GEOM_MULTIPOLYGON>(G, pts, right->d, ix, g, best_d, best_r, cnt, off, left_row_base, pairs_dev, dist_dev, s);
        }
    };
    rc = pass2();
    if (rc != GPK_OK) return done(rc);
    if (host_out) {
        rc = sc_out.copy_back(s);
        if (rc != GPK_OK) return done(rc);
    } else {
        e = hipStreamSynchronize(s);  // (the call is synchronous, like gpk_spatial_join)
        if (e != hipSuccess) return done(fail(GPK_ERR_DEVICE, "nearest_join: %s", hipGetErrorString(e)));
    }
    return done(GPK_OK);
}
