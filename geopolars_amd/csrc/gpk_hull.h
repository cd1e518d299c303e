// gpk_hull.h — the hull stage of gpk_hull.hip for the operators that work on a row's convex hull without emitting it
// (gpk_minbound.hip): every row's exact hull, left in slices of the calling thread's workspace.
#pragma once

#include "gpk_device.h"

namespace gpk {

// the coordinate range [c0, c1) of row g, members and rings included (a NaN point is an empty row)
__device__ __forceinline__ void geom_coord_range(const DevGeo& a, int64_t g, int& c0, int& c1) {
    switch (a.type) {
    case GPK_GEOM_POINT: {
        const double2 p = a.xy[g];
        c0 = (int)g;
        c1 = (isnan(p.x) || isnan(p.y)) ? (int)g : (int)g + 1;
        break;
    }
    case GPK_GEOM_LINESTRING:
    case GPK_GEOM_MULTIPOINT:
        c0 = a.geom_off[g];
        c1 = a.geom_off[g + 1];
        break;
    case GPK_GEOM_POLYGON:
    case GPK_GEOM_MULTILINESTRING:
        c0 = a.ring_off[a.geom_off[g]];
        c1 = a.ring_off[a.geom_off[g + 1]];
        break;
    default:
        c0 = a.ring_off[a.part_off[a.geom_off[g]]];
        c1 = a.ring_off[a.part_off[a.geom_off[g + 1]]];
    }
}

// What the stage leaves for row g whose coordinates are [c0, c1):
//   n_pts[g]   the row's points (the closing duplicate of a ring dropped), -1 for a null row or one without a coordinate;
//   sizes[g]   the coordinates of its CLOSED hull ring (0: no hull; 2: one distinct point p p; 3: collinear p q p; else h + 1);
//   the ring   at hull_slice(stack, c0, g): counter-clockwise from the lexicographically smallest vertex, no collinear vertices.
struct HullStage {
    double2* stack;
    int32_t* sizes;
    int32_t* n_pts;
    // the stage's own temporaries
    double2* sorted;
    int32_t *idx_scratch, *big_list, *mid_list;
};
__host__ __device__ __forceinline__ double2* hull_slice(double2* stack, int c0, int64_t g) { return stack + 2 * (int64_t)c0 + 2 * g; }

// hull_stage_plan adds the stage's carves for a column of n rows and nc coordinates to the caller's Scratch (on workspace()), which the
// caller commits after adding its own; hull_stage then, when the column has rows, launches the hull kernels on s.
void hull_stage_plan(Scratch& sc, int64_t n, int64_t nc, HullStage* h);
int32_t hull_stage(const gpk_geoarray* a, const HullStage& h, hipStream_t s);

}  // namespace gpk
