// gpk_dwithin_refine.h — the per-candidate exact distance kernels of gpk_dwithin.hip with a threshold per LEFT ROW in place of the
// join's one distance: what gpk_nearest_join_any (gpk_nearest_any.hip) computes its seed distances and its candidates' distances
// with.  The kernels, their lane-group sizes, the PD_LARGE_COST list and its second launch are the ones gpk_dwithin_join runs (one
// template over the candidate struct: the instance for a scalar threshold is the code it always was), so a distance written here is
// bit for bit the double gpk_distance_rowwise's per-row kernel gives for the pair.  The launches live in gpk_dwithin.hip.
#pragma once

#include "gpk_common.h"

namespace gpk {

struct RowCands {
    const uint32_t* l;  // left row of candidate c
    const uint32_t* r;  // right row
    int64_t n;
    const double4* lbox;  // the left rows' own boxes
    const double4* rbox;  // the index's boxes of the right rows
    // per left row: the candidate is evaluated when the distance between the two boxes is <= t[l] + margin (boxes_within of
    // gpk_dwithin.hip; NaN: never, INFINITY: always unless a box holds a NaN)
    const double* t;
    uint8_t* hit;                  // per candidate: d <= t[l]
    double* dist;                  // per candidate: d, NaN for a candidate the box test rejected or a row without a coordinate
    unsigned long long* stats;     // join statistics words or nullptr: [2] += candidates, [3] += candidates the box test rejected
    const char *label, *label_large;  // the profile stages of the group launch and of the work-group launch
};

// `large`: cs.n words, `n_large`: one word (zeroed here); both read only when neither column is POINT.  Enqueues on `s`.
int32_t refine_row_candidates(const char* who, const gpk_geoarray* left, const gpk_geoarray* right, const RowCands& cs, uint32_t* large,
                              uint32_t* n_large, hipStream_t s);

}  // namespace gpk
