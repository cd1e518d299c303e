// gpk_geotake.hip — gpk_geoarray_take / gpk_geoarray_filter: select rows of a geometry column on the device.  Contract:
// include/geopolars_hip.h; the rule (source ranges, the locate step, the two payloads): gpk_geotake.h.
//
// Both calls are one schedule over ROW SLOTS.  take: slot i reads source row idx[i] and is output row i.  filter: slot i is source row
// i, and is an output row when the mask keeps it — a dropped slot is an empty row at every level, which the fill's locate step skips,
// so only the row pass needs the compacted row numbers (a scan of the keep flags, on the device).
//   1. count  (one lane per slot): the slot's source range and child count at every level, whether it stays, whether its row is valid;
//      indices outside [0, n) are counted (one atomic per wave that has one).
//   2. scan   (gpk_scan.h) of every level's counts, and of the keep flags of a filter.  Their 64-bit totals and the out-of-range count
//      are gathered into one record and read back once (d2h_small / sync_small): the only wait of the call.  The totals are checked
//      against Arrow's i32 offsets before anything is allocated.
//   3. rows   (one lane per slot): geom_offsets of the output rows, the entries that close every level, the validity flags at their
//      output rows; for POINT columns the 16-byte gather itself.  bitmap: one lane per output byte.
//   4. fill   (one work-group per strip of 1024 output elements, gt::STRIP): the offsets levels below geom_offsets, then the
//      coordinates — geotake_fill_kernel with the two payloads of gpk_geotake.h, each after the level's strip table (one lane per
//      strip bisects for the row of the strip's first element, so that no work-group of the fill begins with a bisection in global
//      memory).
// Every grid is uncapped: one lane per slot, strip or output byte, one work-group per strip; no kernel loops over units.
#include <climits>

#include "gpk_column.h"
#include "gpk_common.h"
#include "gpk_device.h"
#include "gpk_geotake.h"
#include "gpk_scan.h"

namespace gpk {

namespace {

// the offsets levels of a column, outermost first
struct TakeLevels {
    const int32_t* off[gt::MAX_LEVELS];
    int n;
};
TakeLevels levels_of(const DevGeo& d) {
    TakeLevels L{{nullptr, nullptr, nullptr}, 0};
    if (d.type != GPK_GEOM_POINT) L.off[L.n++] = d.geom_off;
    if (d.type == GPK_GEOM_MULTIPOLYGON) L.off[L.n++] = d.part_off;
    if (d.type == GPK_GEOM_POLYGON || d.type == GPK_GEOM_MULTILINESTRING || d.type == GPK_GEOM_MULTIPOLYGON) L.off[L.n++] = d.ring_off;
    return L;
}

struct TakeScratch {  // per slot, per level
    int32_t* src_lo[gt::MAX_LEVELS];
    int32_t* cnt[gt::MAX_LEVELS];
};

__device__ __forceinline__ bool mask_keeps(const uint8_t* __restrict__ mask, int mask_bits, int64_t i) {
    return mask_bits == 1 ? ((mask[i >> 3] >> (i & 7)) & 1) != 0 : mask[i] != 0;
}

// record: [0 .. 2] level totals, [3] rows that stay, [4] indices out of range (counted here; the others by geotake_record_kernel)
__global__ __launch_bounds__(256) void geotake_count_kernel(TakeLevels L, int64_t n_src, const uint8_t* __restrict__ src_validity,
                                                            const long long* __restrict__ idx, const uint8_t* __restrict__ mask, int mask_bits,
                                                            int64_t n_slots, TakeScratch sc, int32_t* __restrict__ keep, uint8_t* __restrict__ ok,
                                                            unsigned long long* __restrict__ record) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool oob = false;
    if (i < n_slots) {
        const long long j = idx ? idx[i] : (long long)i;
        const bool stays = mask ? mask_keeps(mask, mask_bits, i) : true;
        const bool in_range = j >= 0 && j < n_src;
        oob = stays && !in_range;
        int32_t lo[gt::MAX_LEVELS] = {0, 0, 0}, hi[gt::MAX_LEVELS] = {0, 0, 0};
        if (stays && in_range) gt::row_ranges(L.off, L.n, j, lo, hi);  // (the children of a null source row travel too)
        for (int l = 0; l < L.n; ++l) {
            sc.src_lo[l][i] = lo[l];
            sc.cnt[l][i] = hi[l] - lo[l];
        }
        if (L.n == 0) sc.src_lo[0][i] = (stays && in_range) ? (int32_t)j : -1;  // (POINT: the source row, for the row pass)
        if (keep) keep[i] = stays ? 1 : 0;
        ok[i] = (stays && in_range && dev::valid_row(src_validity, j)) ? 1 : 0;
    }
    const unsigned long long b = __ballot(oob);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&record[4], (unsigned long long)__popcll(b));
}

__global__ void geotake_record_kernel(const unsigned long long* __restrict__ t0, const unsigned long long* __restrict__ t1,
                                      const unsigned long long* __restrict__ t2, const unsigned long long* __restrict__ rows,
                                      unsigned long long* __restrict__ record) {
    if (threadIdx.x == 0) {
        record[0] = t0 ? *t0 : 0;
        record[1] = t1 ? *t1 : 0;
        record[2] = t2 ? *t2 : 0;
        record[3] = rows ? *rows : 0;
    }
}

// One lane per slot.  row_at: the output row of a slot that stays (nullptr: the slot's own number).  Lane 0 closes every level.
struct TakeOut {
    int32_t* off[gt::MAX_LEVELS];
    int32_t total[gt::MAX_LEVELS];
};
__global__ __launch_bounds__(256) void geotake_rows_kernel(int n_levels, const int32_t* __restrict__ dst_lo0, const int32_t* __restrict__ row_at,
                                                           const int32_t* __restrict__ keep, const uint8_t* __restrict__ ok, int64_t n_slots,
                                                           int64_t n_out, TakeOut out, uint8_t* __restrict__ ok_out,
                                                           const gt::Bits16* __restrict__ src_xy, const int32_t* __restrict__ src_row,
                                                           gt::Bits16* __restrict__ out_xy) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && n_levels > 0) {
        out.off[0][n_out] = out.total[0];
        for (int l = 1; l < n_levels; ++l) out.off[l][out.total[l - 1]] = out.total[l];
    }
    if (i >= n_slots || (keep && !keep[i])) return;
    const int64_t row = row_at ? (int64_t)row_at[i] : i;
    if (row >= n_out) return;
    if (n_levels > 0) out.off[0][row] = dst_lo0[i];
    if (ok_out) ok_out[row] = ok[i];
    if (out_xy) {  // POINT: the gather itself; a row without a source row is (NaN, NaN)
        const int32_t j = src_row[i];
        gt::Bits16 v{0x7FF8000000000000ull, 0x7FF8000000000000ull};
        if (j >= 0) v = src_xy[j];
        out_xy[row] = v;
    }
}

// byte-per-row flags -> Arrow bitmap (LSB first): one lane per output byte
__global__ __launch_bounds__(256) void geotake_bitmap_kernel(const uint8_t* __restrict__ flags, int64_t n, uint8_t* __restrict__ bitmap) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (n + 7) / 8) return;
    uint32_t v = 0;
    for (int k = 0; k < 8; ++k) {
        const int64_t i = 8 * b + k;
        if (i < n && flags[i]) v |= 1u << k;
    }
    bitmap[b] = (uint8_t)v;
}

// the strip table of one level: one lane per strip
__global__ __launch_bounds__(256) void geotake_strips_kernel(const int32_t* __restrict__ start, int64_t n_slots, int64_t n_strips,
                                                             int32_t* __restrict__ first_row) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_strips) first_row[s] = gt::strip_first_row(start, n_slots, s);
}

// One work-group per strip of gt::STRIP output elements of one level; start: dst_lo of the level above, one entry per slot.
template <class Payload>
__global__ __launch_bounds__(gt::LANES) void geotake_fill_kernel(Payload p, const int32_t* __restrict__ start, int64_t n_slots, int64_t total,
                                                                  const int32_t* __restrict__ first_row, int64_t n_strips) {
    __shared__ int32_t win[gt::WINDOW];
    __shared__ int32_t shift_win[gt::WINDOW];
    const int t = threadIdx.x;
    const int64_t strip = blockIdx.x, e0 = strip * gt::STRIP;
    if (strip >= n_strips || e0 >= total) return;  // (block-uniform)
    const int64_t e_end = e0 + gt::STRIP < total ? e0 + gt::STRIP : total;
    gt::Rows rows = gt::strip_rows(start, n_slots, first_row, strip, n_strips);
    const int64_t w = rows.last - rows.first + 1;
    if (w <= gt::WINDOW) {  // (block-uniform)
        for (int64_t k = t; k < w; k += gt::LANES) {
            const int32_t at = start[rows.first + k];
            win[k] = at;
            shift_win[k] = p.src_lo[rows.first + k] - at;
        }
        __syncthreads();
        rows.win = win;
        rows.shift_win = shift_win;
    }
    typename Payload::T v[gt::PER_LANE];
    const unsigned have = gt::lane_values(p, rows, e0, e_end, t, v);
    if constexpr (Payload::CONSECUTIVE) {
        static_assert(sizeof(typename Payload::T) == 4 && gt::PER_LANE == 4, "one 16-byte store a lane");
        const int64_t e = gt::lane_element<Payload>(e0, t, 0);
        if (have == 0xFu) {
            *reinterpret_cast<int4*>(p.dst + e) = make_int4(v[0], v[1], v[2], v[3]);  // (the level's base is 256-byte aligned, e a multiple of 4)
        } else {
#pragma unroll
            for (int k = 0; k < gt::PER_LANE; ++k)
                if (have & (1u << k)) p.dst[e + k] = v[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < gt::PER_LANE; ++k)
            if (have & (1u << k)) p.dst[gt::lane_element<Payload>(e0, t, k)] = v[k];
    }
}

inline dim3 lanes_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)); }

// idx (take) or mask (filter): exactly one is given, in the caller's memory space (a host one is staged here; the mask has mask_bytes bytes)
int32_t run(const char* op, const gpk_geoarray* a, const long long* idx_in, const uint8_t* mask_in, int mask_bits, size_t mask_bytes, int32_t in_space,
            int64_t n_slots, hipStream_t s, gpk_geoarray** out, int64_t* n_kept) {
    const DevGeo& d = a->d;
    const TakeLevels L = levels_of(d);
    int device = 0;
    (void)hipGetDevice(&device);
    Column col(op, d.type, device, s);
    if (n_slots == 0) {
        GPK_TRY(col.size(0, 0, 0, 0, d.validity != nullptr));
        GPK_TRY(col.zero_offsets());
        if (n_kept) *n_kept = 0;
        col.release(out);
        return GPK_OK;
    }

    // ---- scratch
    Scratch plan(workspace());
    const int64_t n = n_slots, at = (n + 255) / 256;
    const size_t words = (size_t)(n + 1), tot = (size_t)(at + 2);
    const long long* idx;
    const uint8_t* mask;
    plan.stage_in(idx, idx_in, in_space, (size_t)n);
    plan.stage_in(mask, mask_in, in_space, mask_bytes);
    TakeScratch sc{};
    int32_t* dst_lo[gt::MAX_LEVELS] = {nullptr, nullptr, nullptr};
    unsigned long long* btot[gt::MAX_LEVELS + 1] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l < L.n; ++l) {
        plan.add_n(words, sc.src_lo[l], sc.cnt[l], dst_lo[l]);
        plan.add(btot[l], tot);
    }
    if (L.n == 0) plan.add(sc.src_lo[0], words);  // (POINT: the source row of every slot; idx and mask are not read after the wait)
    int32_t *keep, *row_at;
    plan.add_if(mask_in != nullptr, keep, words);
    plan.add_if(mask_in != nullptr, row_at, words);
    plan.add_if(mask_in != nullptr, btot[gt::MAX_LEVELS], tot);
    uint8_t *ok, *ok_rows;  // ok_rows: the flags at their output rows
    unsigned long long* record;
    plan.add(ok, (size_t)n);
    plan.add_if(mask_in != nullptr, ok_rows, (size_t)n);
    plan.add(record, 32);
    GPK_TRY(plan.commit());
    if (!mask_in) ok_rows = ok;
    GPK_TRY(plan.upload(s));

    // ---- 1, 2: count, scan, the one read-back
    GPK_HIP(hipMemsetAsync(record, 0, 64, s));
    GPK_LAUNCH("gpk_geotake_count", geotake_count_kernel, lanes_grid(n), dim3(256), 0, s, L, d.n_geoms, d.validity, idx, mask, mask_bits, n, sc, keep, ok,
               record);
    for (int l = 0; l < L.n; ++l) GPK_TRY(exclusive_scan_i32(sc.cnt[l], n, dst_lo[l], nullptr, btot[l], s));
    if (mask) GPK_TRY(exclusive_scan_i32(keep, n, row_at, nullptr, btot[gt::MAX_LEVELS], s));
    GPK_LAUNCH("gpk_geotake_totals", geotake_record_kernel, dim3(1), dim3(64), 0, s, L.n > 0 ? btot[0] + at : nullptr, L.n > 1 ? btot[1] + at : nullptr,
               L.n > 2 ? btot[2] + at : nullptr, mask ? btot[gt::MAX_LEVELS] + at : nullptr, record);
    unsigned long long rec[5] = {0, 0, 0, 0, 0};
    GPK_HIP(d2h_small(rec, record, sizeof rec, s));
    GPK_HIP(sync_small(s));
    const int64_t n_out = mask ? (int64_t)rec[3] : n;
    if (n_kept) *n_kept = n_out;
    if (rec[0] > (unsigned long long)INT32_MAX || rec[1] > (unsigned long long)INT32_MAX || rec[2] > (unsigned long long)INT32_MAX)
        return fail(GPK_ERR_INVALID_ARGUMENT, "%s: the result exceeds 2^31 - 1 parts / rings / coordinates (Arrow i32 offsets)", op);

    // ---- the result column: totals by level -> the counts of the type
    const int64_t n_coords = L.n == 0 ? n_out : (int64_t)rec[L.n - 1];
    const int64_t n_parts = d.type == GPK_GEOM_MULTIPOLYGON ? (int64_t)rec[0] : 0;
    const int64_t n_rings = L.n >= 2 ? (int64_t)rec[L.n - 2] : 0;
    const bool validity = d.validity != nullptr || rec[4] > 0;
    GPK_TRY(col.size(n_out, n_parts, n_rings, n_coords, validity));
    TakeOut to{{nullptr, nullptr, nullptr}, {0, 0, 0}};
    {
        int l = 0;
        if (col.geom_off()) to.off[l++] = col.geom_off();
        if (col.part_off()) to.off[l++] = col.part_off();
        if (col.ring_off()) to.off[l++] = col.ring_off();
        for (l = 0; l < L.n; ++l) to.total[l] = (int32_t)rec[l];
    }

    // ---- 3: rows, bitmap
    const bool point = L.n == 0;
    GPK_LAUNCH("gpk_geotake_rows", geotake_rows_kernel, lanes_grid(n), dim3(256), 0, s, L.n, (const int32_t*)dst_lo[0], (const int32_t*)row_at,
               (const int32_t*)keep, (const uint8_t*)ok, n, n_out, to, (validity && mask) ? ok_rows : (uint8_t*)nullptr,
               point ? (const gt::Bits16*)d.xy : (const gt::Bits16*)nullptr, (const int32_t*)sc.src_lo[0], point ? (gt::Bits16*)col.xy() : (gt::Bits16*)nullptr);
    if (validity && n_out > 0)
        GPK_LAUNCH("gpk_geotake_bitmap", geotake_bitmap_kernel, lanes_grid((n_out + 7) / 8), dim3(256), 0, s, (const uint8_t*)ok_rows, n_out, col.validity());

    // ---- 4: fill — level l's entries are located through the row starts of level l - 1, the coordinates through the last level's.
    // The strip tables are sized by the totals: a second arena (the first one's carves stay valid).
    int64_t n_strips[gt::MAX_LEVELS] = {0, 0, 0};  // [l]: of the elements located through dst_lo[l]
    int32_t* first_rows[gt::MAX_LEVELS];
    Scratch tables(workspace_aux(0));
    for (int l = 0; l < L.n; ++l) {
        n_strips[l] = ((int64_t)rec[l] + gt::STRIP - 1) / gt::STRIP;
        tables.add_if(rec[l] > 0, first_rows[l], (size_t)(n_strips[l] + 1));
    }
    GPK_TRY(tables.commit());
    for (int l = 0; l < L.n; ++l) {
        const int64_t total = (int64_t)rec[l];
        if (total == 0) continue;
        int32_t* first_row = first_rows[l];
        GPK_LAUNCH("gpk_geotake_strips", geotake_strips_kernel, lanes_grid(n_strips[l]), dim3(256), 0, s, (const int32_t*)dst_lo[l], n, n_strips[l], first_row);
        const dim3 grid((unsigned)n_strips[l]);
        if (l + 1 < L.n) {
            const gt::OffsetPayload p{L.off[l + 1], to.off[l + 1], sc.src_lo[l], sc.src_lo[l + 1], dst_lo[l + 1]};
            GPK_LAUNCH("gpk_geotake_offsets", geotake_fill_kernel<gt::OffsetPayload>, grid, dim3(gt::LANES), 0, s, p, (const int32_t*)dst_lo[l], n, total,
                       (const int32_t*)first_row, n_strips[l]);
        } else {
            const gt::CoordPayload p{(const gt::Bits16*)d.xy, (gt::Bits16*)col.xy(), sc.src_lo[l]};
            GPK_LAUNCH("gpk_geotake_coords", geotake_fill_kernel<gt::CoordPayload>, grid, dim3(gt::LANES), 0, s, p, (const int32_t*)dst_lo[l], n, total,
                       (const int32_t*)first_row, n_strips[l]);
        }
    }
    col.release(out);
    return GPK_OK;
}

}  // namespace

}  // namespace gpk

using namespace gpk;

extern "C" {

int32_t gpk_geoarray_take(const gpk_geoarray* a, const int64_t* idx, int64_t n_idx, int32_t idx_space, void* stream, gpk_geoarray** out) {
    if (out) *out = nullptr;
    if (!a || !out) return fail(GPK_ERR_INVALID_ARGUMENT, "geoarray_take: NULL argument");
    if (n_idx < 0 || n_idx > (int64_t)INT32_MAX) return fail(GPK_ERR_INVALID_ARGUMENT, "geoarray_take: %lld indices", (long long)n_idx);
    if (n_idx > 0 && !idx) return fail(GPK_ERR_INVALID_ARGUMENT, "geoarray_take: idx is NULL");
    if (idx_space != GPK_MEM_HOST && idx_space != GPK_MEM_DEVICE) return fail(GPK_ERR_INVALID_ARGUMENT, "geoarray_take: unknown memory space %d", idx_space);
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    return run("geoarray_take", a, (const long long*)idx, nullptr, 0, 0, idx_space, n_idx, s, out, nullptr);
}

int32_t gpk_geoarray_filter(const gpk_geoarray* a, const uint8_t* mask, int32_t mask_bits, int32_t mask_space, void* stream, gpk_geoarray** out,
                            int64_t* n_kept) {
    if (out) *out = nullptr;
    if (n_kept) *n_kept = 0;
    if (!a || !out || !n_kept) return fail(GPK_ERR_INVALID_ARGUMENT, "geoarray_filter: NULL argument");
    if (mask_bits != 1 && mask_bits != 8)
        return fail(GPK_ERR_INVALID_ARGUMENT, "geoarray_filter: a mask of %d bits a row (1: Arrow bitmap, 8: a byte a row)", mask_bits);
    if (mask_space != GPK_MEM_HOST && mask_space != GPK_MEM_DEVICE)
        return fail(GPK_ERR_INVALID_ARGUMENT, "geoarray_filter: unknown memory space %d", mask_space);
    const int64_t n = a->d.n_geoms;
    if (n > 0 && !mask) return fail(GPK_ERR_INVALID_ARGUMENT, "geoarray_filter: mask is NULL");
    GPK_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const size_t mask_bytes = mask_bits == 1 ? (size_t)((n + 7) / 8) : (size_t)n;
    return run("geoarray_filter", a, nullptr, mask, mask_bits, mask_bytes, mask_space, n, s, out, n_kept);
}

}  // extern "C"
