// gpk_column.h — a result column the library owns, while it is under construction: the handle of gpk_line_clip, gpk_polygon_clip,
// gpk_polygon_union, gpk_allgatherv_geoarray and gpk_geoarray_concat from its creation until the caller gets it.  Defined in
// gpk_runtime.hip, beside gpk_geoarray_free.  (gpk_geoarray_upload mixes borrowed and owned levels and the WKB decoder takes its
// buffers from the block cache: both build their handles themselves.)
#pragma once

#include "gpk_common.h"

namespace gpk {

class Column {
  public:
    // op: the operation's name in error messages
    Column(const char* op, int32_t type, int device, hipStream_t s);
    // an unreleased column (an error return): waits for the stream — work queued on it may still write the buffers — and frees the handle
    ~Column();
    Column(const Column&) = delete;
    Column& operator=(const Column&) = delete;

    // The one sizing call: fills the view's counts (n_parts as given for MULTIPOLYGON, else n_geoms for polygonal types, else 0; n_rings
    // only where the type has a ring level) and allocates exactly the levels the type has (device_malloc; a level of zero bytes still
    // gets 8) plus, when asked, a validity bitmap of n_geoms bits.  Returns the status: a caller may have to carry it elsewhere.
    int32_t size(int64_t n_geoms, int64_t n_parts, int64_t n_rings, int64_t n_coords, bool validity);
    // the first entry of every offsets level present := 0 (stream-ordered): all there is to write when the column has no rows
    int32_t zero_offsets();

    double2* xy() { return (double2*)a_->owned[0]; }
    int32_t* geom_off() { return (int32_t*)a_->owned[1]; }
    int32_t* part_off() { return (int32_t*)a_->owned[2]; }
    int32_t* ring_off() { return (int32_t*)a_->owned[3]; }
    uint8_t* validity() { return (uint8_t*)a_->owned[4]; }
    int64_t nbytes() const { return a_->nbytes; }

    void release(gpk_geoarray** out) {
        *out = a_;
        a_ = nullptr;
    }

  private:
    const char* op_;
    hipStream_t s_;
    gpk_geoarray* a_;
};

}  // namespace gpk
