// gpk_candjoin.h — the staged bbox candidate generator of gpk_join.hip (bbox_join: candidates per left box from the right side's grid
// directory, a per-candidate refine, then count / scan / emit of the hits sorted by (l, r)) opened to a refine that lives in another
// translation unit.  The within-distance join (gpk_dwithin.hip) hands over left boxes grown by its distance and refines every
// candidate with the library's distance routines.
#pragma once

#include "gpk_index.h"

namespace gpk {

struct CandRefine {
    const char* name;  // the calling entry point, for error messages ("dwithin_join")
    void* ctx;
    // scratch per call, carved from the candidate arena next to the candidate lists: fixed + per_cand * n_candidates bytes
    size_t scratch_fixed, scratch_per_cand;
    // fills hit[0 .. n_cand) for the candidates (cand_l[c], cand_r[c]) (left row ascending, right row ascending within a left row);
    // `stats`: the join statistics words (gpk_join_stats) or nullptr when they are off
    int32_t (*refine)(void* ctx, const uint32_t* cand_l, const uint32_t* cand_r, int32_t n_cand, void* scratch, uint8_t* hit,
                      unsigned long long* stats, hipStream_t s);
    // enqueued after the pairs were emitted: row i's hits, in candidate order, are pairs offsets[i] .. of the output (a per-pair
    // payload is gathered here); nullptr: nothing to gather.  Only called when pairs were asked for.
    int32_t (*emitted)(void* ctx, int64_t n_rows, const int32_t* cand_off, const uint8_t* hit, const int32_t* offsets, void* scratch,
                       int64_t pair_capacity, hipStream_t s);
};

// bbox_join of gpk_join.hip with the caller's left boxes (device, one per left row; NaN: no candidates) and the caller's refine.
// Outputs, capacity rule and errors as gpk_spatial_join; uses workspace() and workspace_aux(1), leaves workspace_aux(0) alone.
int32_t bbox_join_refined(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, uint32_t left_row_base,
                          uint32_t* out_counts, uint32_t* out_pairs, int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, hipStream_t s,
                          const double4* lbbox, const CandRefine& refine);

}  // namespace gpk
