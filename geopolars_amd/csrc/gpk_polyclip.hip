// gpk_polyclip.hip — polygon x polygon intersection and difference: gpk_polygon_clip over the routines of gpk_polyclip.h.  Contract:
// include/geopolars_hip.h; the rule: gpk_polyclip.h; the schedule (count -> scan -> fill -> stitch -> scan -> emit, the kernels and
// the host driver, shared with gpk_polygon_union): gpk_polyclip_run.h, here with the kept table of the two clip modes.
#include "gpk_polyclip_run.h"

using namespace gpk;

extern "C" int32_t gpk_polygon_clip(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows,
                                    int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status,
                                    int32_t status_space, void* stream, gpk_geoarray** out) {
    static const RunNames names = {"polygon_clip",           "gpk_polygon_clip_count",   "gpk_polygon_clip_fill", "gpk_polygon_clip_stitch",
                                   "gpk_polygon_clip_totals", "gpk_polygon_clip_offsets", "gpk_polygon_clip_emit"};
    return polygon_clip_run<pc::ClipRule, false>(names, mode == GPK_PCLIP_INTERSECTION || mode == GPK_PCLIP_DIFFERENCE, a, b, a_rows, b_rows, n_rows,
                                                 rows_space, mode, flags, out_src, src_space, out_status, status_space, stream, out);
}
