// gpk_candjoin.h — what the joins share: the staged bbox candidate generator of gpk_bboxjoin.hip (bbox_join: candidates per left box from
// the right side's grid directory, a per-candidate refine, then count / scan / emit of the hits sorted by (l, r)) with its one refine
// interface, the driver of the joins that return a value per pair (payload_join, gpk_bboxjoin.hip), the host steps every pairs join
// repeats and those of the row-wise relation calls (rowwise_pairs).  The predicates of gpk_spatial_join refine with the kernels of
// gpk_bboxjoin.hip; the relation, measure and within-distance joins bring their own refine to payload_join, the last with left boxes
// grown by its distance.
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
    // enqueued last, when pairs were asked for: `pairs` is the DEVICE pair buffer (the caller's, or its staging) holding row i's hits in
    // candidate order at offsets[i] — a join that orders a row's pairs itself (gpk_knn.hip: by rank) rewrites them here.  nullptr
    // (every other join): the pairs stay as emitted.
    int32_t (*emitted_pairs)(void* ctx, const int32_t* offsets, uint32_t left_row_base, uint32_t* pairs, int64_t pair_capacity, hipStream_t s);
};

// The box-candidate join with the caller's left boxes (device, one per left row; NaN: no candidates; nullptr: the rows' own boxes,
// computed with gpk_bounds) and the caller's refine.  Outputs, capacity rule and errors as gpk_spatial_join; uses workspace() and
// workspace_aux(1), leaves workspace_aux(0) alone unless it computes the boxes itself.
int32_t bbox_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, uint32_t left_row_base,
                  uint32_t* out_counts, uint32_t* out_pairs, int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, hipStream_t s,
                  const double4* lbbox, const CandRefine& refine);
// the rows' own boxes in workspace_aux(0), for a caller whose refine reads the boxes it hands to bbox_join
int32_t left_boxes(const gpk_geoarray* left, hipStream_t s, const double4** out);

// The refines of gpk_spatial_join (gpk_bboxjoin.hip) over one context: the two columns, the boxes bbox_join is handed and the index's
// boxes of the right rows.  The lineal x point refine reads no boxes (lbbox may be nullptr).
struct BoxRefineCtx {
    const gpk_geoarray *left, *right;
    const double4 *lbbox, *rbbox;
    bool l_one_ring, r_one_ring;  // every polygon of that POLYGON column is known to have exactly one ring
};
// (filled AFTER the left boxes were computed: gpk_bounds classifies the column's rings, which is where l_one_ring comes from)
BoxRefineCtx box_refine_ctx(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, const double4* lbbox);
CandRefine polygonal_intersects_refine(BoxRefineCtx* cx);
CandRefine polygonal_contains_refine(BoxRefineCtx* cx);
CandRefine lineal_point_refine(BoxRefineCtx* cx);

// ---- joins that return a value per pair -----------------------------------------------------------------------------------------
// The relation joins (gpk_polyrel.hip, gpk_lineline.hip, gpk_linearea.hip: a uint8 mask), the measure join (gpk_overlay.hip: a double)
// and the within-distance join (gpk_dwithin.hip: a double) are bbox_join with a payload: the refine leaves one element per CANDIDATE
// in its scratch — 256 bytes it may use as it likes, then payload[n_cand] — and after the emit the hits' elements are gathered into
// the caller's buffer, in pair order.  A family's refine context begins with this:
struct PayloadCtx {
    const gpk_geoarray *left, *right;
    const char* gather_label;  // the profile stage of the gather ("gpk_polygon_relation_gather")
    size_t payload_elem;       // bytes per element: 1 or 8
    void* payload_out;         // set by payload_join — device: the caller's buffer or its staging; nullptr: no payload asked for
};
struct PayloadJoin {
    const char* who;  // the calling entry point, for error messages
    PayloadCtx* ctx;  // what the refine and the hook below get as `ctx`
    decltype(CandRefine::refine) refine;
    size_t extra_per_cand;  // scratch per candidate behind the payload
    // nullptr: candidates from the left rows' own boxes.  Otherwise called once `own` (those boxes) is enqueued and the right side's
    // index exists: it fills `other` (n boxes), which take the left boxes' place in the candidate search.
    int32_t (*boxes)(PayloadCtx* ctx, const gpk_index* right_index, const double4* own, double4* other, int64_t n, hipStream_t s);
    // nullptr: the payload of a row's hits is gathered in candidate order.  Otherwise CandRefine::emitted_pairs of a join that writes
    // pairs and payload (PayloadCtx::payload_out, nullptr when none was asked for) in an order of its own; the gather does not run.
    decltype(CandRefine::emitted_pairs) emitted_pairs = nullptr;
};
// Everything such a join does once its arguments are validated: the empty cases, a temporary GPK_INDEX_BBOX_GRID index when the caller
// has none (freed on every path, after a sync), boxes and payload staging in workspace_aux(0), bbox_join, the payload of a host caller.
int32_t payload_join(const PayloadJoin& join, const gpk_index* right_index, uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs,
                     void* out_payload, int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream);

// gpk_join.hip: the join statistics words, or nullptr unless gpk_join_stats_enable(1)
unsigned long long* join_stats_buffer();

// ---- host steps of every pairs join ---------------------------------------------------------------------------------------------
// (an index whose slabs name coordinates by index reads THIS array's coordinates: rows alone do not identify the column)
inline int32_t index_matches(const gpk_index* right_index, const gpk_geoarray* right) {
    if (right_index->n_geoms != right->d.n_geoms || right_index->n_coords != right->d.n_coords || right_index->n_rings != right->d.n_rings)
        return fail(GPK_ERR_INVALID_ARGUMENT, "right_index was built over a different array");
    return GPK_OK;
}
inline int32_t index_matches_with_grid(const gpk_index* right_index, const gpk_geoarray* right, const char* who) {
    GPK_TRY(index_matches(right_index, right));
    if (!right_index->v.grid || !right_index->v.cell_off || !right_index->v.items || !right_index->v.bbox)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: right_index carries no bbox grid", who);
    return GPK_OK;
}

// an empty join: every count is zero (enqueued on `s` for a device caller)
inline int32_t zero_counts(uint32_t* out_counts, int64_t n, int32_t out_space, hipStream_t s) {
    if (!out_counts || n <= 0) return GPK_OK;
    if (out_space == GPK_MEM_DEVICE)
        GPK_HIP(hipMemsetAsync(out_counts, 0, sizeof(uint32_t) * (size_t)n, s));
    else
        memset(out_counts, 0, sizeof(uint32_t) * (size_t)n);
    return GPK_OK;
}

// The end of a pairs join whose total is on the host: *n_pairs, then — for a host caller — the n counts and the first
// min(total, pair_capacity) pairs from their device staging, then the capacity error.
inline int32_t finish_pairs(const char* who, int64_t total, int64_t n, uint32_t* out_counts, const uint32_t* counts_dev, uint32_t* out_pairs,
                            const uint32_t* pairs_dev, int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, hipStream_t s) {
    *n_pairs = total;
    if (out_space != GPK_MEM_DEVICE) {
        if (out_counts) GPK_TRY(copy_out(out_counts, out_space, counts_dev, sizeof(uint32_t) * (size_t)n, s));
        if (pair_capacity > 0)
            GPK_TRY(copy_out(out_pairs, out_space, pairs_dev, sizeof(uint32_t) * 2 * (size_t)(total < pair_capacity ? total : pair_capacity), s));
    }
    if (pair_capacity > 0 && total > pair_capacity)
        return fail(GPK_ERR_CAPACITY, "%s: %lld pairs but capacity %lld", who, (long long)total, (long long)pair_capacity);
    return GPK_OK;
}

// ---- host steps of a row-wise call over two columns -----------------------------------------------------------------------------
// What gpk_polygon_relation, gpk_line_relation, gpk_line_polygon_relation and gpk_intersection_measure do after their family check:
// out[i] (`elem` bytes) for row i of a against row b_rows[i] (or i) of b.  A host caller's `out` and `b_rows` are staged in
// workspace(); `launch(rows_dev, out_dev, n, s)` enqueues the family's kernel on device pointers.
template <typename Launch>
inline int32_t rowwise_pairs(const char* who, const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, void* out, size_t elem,
                             int32_t out_space, void* stream, Launch launch) {
    const int64_t n = a->d.n_geoms;
    if (!b_rows && n != b->d.n_geoms)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: row counts differ (%lld vs %lld)", who, (long long)n, (long long)b->d.n_geoms);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return GPK_OK;
    const size_t ob = elem * (size_t)n;
    Scratch sc(workspace());
    uint8_t* out_dev;
    const uint32_t* rows_dev;
    sc.stage(out_dev, (uint8_t*)out, out_space, ob);
    sc.stage_in(rows_dev, b_rows, out_space, (size_t)n);
    GPK_TRY(sc.commit());
    GPK_TRY(sc.upload(s));
    GPK_TRY(launch(rows_dev, (void*)out_dev, n, s));
    return copy_out(out, out_space, out_dev, ob, s);
}

}  // namespace gpk
