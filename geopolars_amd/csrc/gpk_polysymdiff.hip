// gpk_polysymdiff.hip — polygon x polygon symmetric difference: gpk_polygon_symdiff, the schedule of gpk_polyclip_run.h instantiated
// with the table of gpk_polysymdiff.h (directions by class, junctions at crossings) and the innermost-shell nesting: its own count,
// fill and stitch kernels; gpk_polygon_clip and gpk_polygon_union launch what they launched.  Contract: include/geopolars_hip.h.
#include "gpk_polyclip_run.h"
#include "gpk_polysymdiff.h"

using namespace gpk;

extern "C" int32_t gpk_polygon_symdiff(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows,
                                       int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status,
                                       int32_t status_space, void* stream, gpk_geoarray** out) {
    static const RunNames names = {"polygon_symdiff",           "gpk_polygon_symdiff_count",   "gpk_polygon_symdiff_fill", "gpk_polygon_symdiff_stitch",
                                   "gpk_polygon_symdiff_totals", "gpk_polygon_symdiff_offsets", "gpk_polygon_symdiff_emit"};
    return polygon_clip_run<ps::SymdiffRule, true>(names, mode == GPK_PSYMDIFF_SYMMETRIC_DIFFERENCE, a, b, a_rows, b_rows, n_rows, rows_space, mode, flags,
                                                   out_src, src_space, out_status, status_space, stream, out);
}
