/*
 * geopolars_hip.h — flat C ABI of libgeopolars_hip.so, the MI355X (gfx950) geometry-kernel
 * backend that sits under GeoPolars' `GeoSeries` operator surface.
 *
 * Every entry point replaces one `todo!()` body (or one dead-code call site) in the reference:
 *   trait GeoSeries / impl GeoSeries for Series   geopolars/geopolars-geo/src/geoseries.rs:10-181,183-279
 *   spatial_join + SpatialIndex                    geopolars/src/spatial_index.rs:37-204,314-350
 *   row codec (WKB <-> geometry)                   geopolars/geopolars-geo/src/util.rs:11-37
 * The only FFI convention the reference has is the Arrow C Data Interface
 * (py-geopolars/src/ffi.rs:12-52): single-chunk arrays, inputs BORROWED for the call, outputs owned
 * by the producer until released.  This ABI keeps that ownership model but speaks raw GeoArrow
 * buffers (coords FixedSizeList<f64,2> interleaved + i32 List offsets) so a Rust shim can pass
 * `array.values().as_ptr()` straight through (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - All functions return int32_t status (GPK_OK == 0).  Nothing throws or aborts across the ABI;
 *     `gpk_last_error` returns a thread-local message.  Status codes map onto
 *     `GeopolarsError` (geopolars/geopolars-geo/src/error.rs:9-28) in the shim.
 *   - Pointers carry a memory space tag (GPK_MEM_HOST / GPK_MEM_DEVICE).  Host buffers are copied to
 *     HBM once by `gpk_geoarray_upload`; device buffers are borrowed (zero copy) — that is how a
 *     caller that already holds data in HBM (another kernel, a torch tensor's data_ptr) plugs in.
 *   - `stream` is a hipStream_t passed as void* (NULL = HIP's legacy default stream, which orders
 *     against every other blocking stream of the device; pass your own stream for concurrency).
 *     Calls with host outputs block until the result is host-visible; calls with device outputs are
 *     stream-ordered and do not synchronise.
 *   - Geometry handles are immutable after upload and may be shared between threads
 *     (mirrors `Arc<SpatialIndex>`, spatial_index.rs:20-21).
 *   - Null rows: validity bitmaps are Arrow LSB-first; null in -> null out (never a panic, unlike
 *     util.rs:32).
 *   - There is NO CPU fallback in this library.  Without a gfx950 device every compute entry point
 *     returns GPK_ERR_DEVICE.
 */
#ifndef GEOPOLARS_HIP_H
#define GEOPOLARS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define GPK_OK                        0
#define GPK_ERR_MISMATCHED_GEOMETRY   1 /* -> GeopolarsError::MismatchedGeometry (error.rs:12-16) */
#define GPK_ERR_INVALID_OFFSETS       2 /* -> PolarsError::ComputeError */
#define GPK_ERR_NULL_UNSUPPORTED      3
#define GPK_ERR_DEVICE                4 /* HIP error / no device / extension not usable */
#define GPK_ERR_OOM                   5
#define GPK_ERR_INVALID_ARGUMENT      6
#define GPK_ERR_CAPACITY              7 /* caller-provided pair buffer too small; n_pairs is set */

/* ---- geometry type ids: identical to GeoSeries::geom_type (geoseries.rs:60-73) --------------- */
#define GPK_GEOM_POINT             0
#define GPK_GEOM_LINESTRING        1
#define GPK_GEOM_POLYGON           3
#define GPK_GEOM_MULTIPOINT        4
#define GPK_GEOM_MULTILINESTRING   5
#define GPK_GEOM_MULTIPOLYGON      6

#define GPK_MEM_HOST    0
#define GPK_MEM_DEVICE  1

/* ---- predicates: `Predicate` of spatial_index.rs:13,28 -------------------------------------- */
#define GPK_PRED_INTERSECTS  0 /* default, spatial_index.rs:28 */
#define GPK_PRED_CONTAINS    1
#define GPK_PRED_WITHIN      2 /* within(a,b) == contains(b,a) */

/*
 * One single-chunk GeoArrow array.  Nesting by type:
 *   POINT                         coords
 *   LINESTRING / MULTIPOINT       geom_offsets[n+1] -> coords
 *   POLYGON / MULTILINESTRING     geom_offsets[n+1] -> rings ; ring_offsets[n_rings+1] -> coords
 *   MULTIPOLYGON                  geom_offsets[n+1] -> parts ; part_offsets[n_parts+1] -> rings ;
 *                                 ring_offsets[n_rings+1] -> coords
 * coords are interleaved xy (FixedSizeList<f64,2>) — or SEPARATED: `xy` NULL and `x`, `y` two arrays of n_coords doubles, the
 * Struct<x: f64, y: f64> coordinate arrays the reference's Python layer builds with `pyarrow.StructArray.from_arrays([x, y])`
 * (py-geopolars/python/geopolars/internals/geoseries.py:86-113).  Kernels read interleaved coordinates (one 16-byte request per
 * vertex); a separated descriptor is interleaved ON THE DEVICE while it is uploaded — one pass, no host-side copy — so the
 * handle owns its coordinates even when the descriptor's buffers are device memory (offsets and validity are still borrowed).
 * Rings are stored closed (first == last).  Unused offset pointers are NULL.  All buffers of one descriptor live in `mem_space`.
 */
typedef struct gpk_geoarrow_desc {
    int32_t        geom_type;     /* GPK_GEOM_* */
    int32_t        mem_space;     /* GPK_MEM_HOST or GPK_MEM_DEVICE */
    int64_t        n_geoms;
    int64_t        n_coords;
    const double*  xy;            /* 2*n_coords doubles */
    const int32_t* geom_offsets;  /* n_geoms+1 or NULL (POINT) */
    const int32_t* part_offsets;  /* n_parts+1, MULTIPOLYGON only */
    const int32_t* ring_offsets;  /* n_rings+1, POLYGON / MULTILINESTRING / MULTIPOLYGON */
    int64_t        n_parts;       /* MULTIPOLYGON only */
    int64_t        n_rings;       /* POLYGON / MULTILINESTRING / MULTIPOLYGON */
    const uint8_t* validity;      /* Arrow bitmap, NULL = all valid */
    const double*  x;             /* separated coordinates (xy == NULL): n_coords doubles each, else NULL */
    const double*  y;
} gpk_geoarrow_desc;

typedef struct gpk_geoarray gpk_geoarray; /* device-resident SoA copy (or borrowed view) */
typedef struct gpk_index    gpk_index;    /* device-resident spatial index over one geoarray */

/* ---- library ------------------------------------------------------------------------------ */
const char* gpk_version(void);
int32_t gpk_last_error(char* buf, size_t cap);
int32_t gpk_device_count(int32_t* out_n);
/* name + CU count of the current HIP device; fails with GPK_ERR_DEVICE when it is not gfx950 */
int32_t gpk_device_info(char* name_buf, size_t cap, int32_t* out_cus);
/* Index tables and build temporaries are recycled through a cache of device blocks inside the library (a freed index's tables serve
 * the next build: SpatialIndex values come and go with the dataframe pipeline, spatial_index.rs:37-71, and hipMalloc / hipFree of
 * gigabytes cost up to hundreds of milliseconds).  The cache holds at most GPK_DEVICE_CACHE_MB (default: a sixteenth of the device's
 * memory, 16 GB at most; 0 = no cache); this call hands every idle block back to the driver now. */
int32_t gpk_device_cache_release(void);

/* ---- "copied once to HBM as SoA" ---------------------------------------------------------- */
/* replaces the per-op row decode of util.rs:27-37 (iter_geom).  A DEVICE view whose offsets do not start at 0 (a sliced Arrow list
 * array: unrebased offsets next to the slice of the child buffer they index) is accepted: the level gets an owned, rebased copy, so
 * every entry point sees children indexed from 0 (one 4-byte read-back per offsets level and upload of a device view). */
int32_t gpk_geoarray_upload(const gpk_geoarrow_desc* desc, void* stream, gpk_geoarray** out);
int32_t gpk_geoarray_free(gpk_geoarray* a);
/* A handle derives tables from its OFFSETS on first use and keeps them (the size classes of the streaming reductions, the strip table and
 * ring records of their one-pass form: csrc/gpk_unary.hip, csrc/gpk_ringstream.hip) — handles are immutable (above).  A handle over
 * BORROWED device buffers (GPK_MEM_DEVICE descriptors) is only as immutable as its owner keeps those buffers: rewriting COORDINATES in
 * place is harmless to the tables, rewriting OFFSETS is not — call this (or make a new handle: no copy either way) before the next
 * call on the handle.  Waits for the handle's device.  No other call on the handle may be in flight on any thread.  (The index
 * gpk_spatial_join keeps on a handle is kept only on handles that own their buffers: nothing to drop there.) */
int32_t gpk_geoarray_invalidate(gpk_geoarray* a);
/* HBM bytes held by the handle (owned + borrowed), for roofline accounting */
int32_t gpk_geoarray_nbytes(const gpk_geoarray* a, int64_t* out_bytes);

/* WKB BinaryArray<i32> (util.rs:27-37 input format) -> GeoArrow buffers, host side (both byte orders; Z / M ordinates are read past).
 * Pass 1 (out == NULL): validates and fills `counts` = {geom_type, n_geoms, n_parts, n_rings, n_coords}.
 * Pass 2: fills caller-allocated buffers of exactly those sizes.  Mixed Polygon/MultiPolygon input is
 * promoted to MULTIPOLYGON, mixed LineString/MultiLineString to MULTILINESTRING. */
int32_t gpk_wkb_decode(const uint8_t* wkb_values, const int32_t* wkb_offsets, int64_t n_rows,
                       const uint8_t* validity, int64_t counts[5], double* xy,
                       int32_t* geom_offsets, int32_t* part_offsets, int32_t* ring_offsets);

/* The same decode on the GPU: the raw WKB column (values + offsets, in `mem_space`) is copied to HBM once and
 * decoded there into a device-resident handle (scan -> prefix sums -> fill); the GeoArrow SoA never exists on
 * the host.  Little-endian ISO WKB / EWKB+SRID, 2D, types 1-6, same promotion rules as gpk_wkb_decode.  A HOST column that also
 * holds big-endian records or Z / M ordinates (EWKB flags, ISO 1000-codes) is parsed by the host decoder instead — both byte orders,
 * Z / M dropped like geozero's to_geo drops them for the reference — and uploaded: same handle, without the GPU's parse rate; in a
 * DEVICE column such rows are reported (GPK_ERR_MISMATCHED_GEOMETRY).  Type 7 (GeometryCollection, geoseries.rs:60-73) has no GeoArrow
 * nesting and is reported either way. */
int32_t gpk_geoarray_from_wkb(const uint8_t* wkb_values, const int32_t* wkb_offsets, int64_t n_rows,
                              const uint8_t* validity, int32_t mem_space, void* stream,
                              gpk_geoarray** out, int32_t* out_geom_type);
/* GeoArrow -> WKB BinaryArray<i32>: the column format geometry-valued results leave the reference in
 * (from_geom_vec, util.rs:11-24).  Little-endian ISO WKB, 2D, one WKB type per column (the array's), zero-length
 * records for null rows (the validity bitmap travels separately).
 *   out_offsets[n_geoms + 1]   Arrow offsets (may be NULL)
 *   out_values[capacity]       WKB bytes (NULL + capacity 0 = size query)
 *   *n_bytes                   total bytes, always set; GPK_ERR_CAPACITY when > capacity, or when the column
 *                              cannot fit i32 offsets (encode row slices)
 * gpk_wkb_encode: host buffers in, host buffers out, no device.  gpk_geoarray_to_wkb: encodes a device-resident
 * handle ON the GPU (sizes -> scan -> headers -> bodies); outputs in `out_space`. */
int32_t gpk_wkb_encode(const gpk_geoarrow_desc* desc, int32_t* out_offsets, uint8_t* out_values,
                       int64_t capacity, int64_t* n_bytes);
int32_t gpk_geoarray_to_wkb(const gpk_geoarray* a, int32_t* out_offsets, uint8_t* out_values,
                            int64_t capacity, int64_t* n_bytes, int32_t out_space, void* stream);
/* The reference's FFI seam — the Arrow C Data Interface (py-geopolars/src/ffi.rs:12-32: a pyarrow array exported with `_export_to_c`,
 * rechunked to ONE array first, :56) — as an entry point: `array` / `schema` are the two exported structs of a geometry column in
 * host memory, BORROWED for the call (the caller releases them as it would after any import).  Accepted columns
 *   Binary / LargeBinary ("z" / "Z")                     WKB rows: decoded on the GPU like gpk_geoarray_from_wkb
 *   [List<]* Struct<x: f64, y: f64>                       native GeoArrow with SEPARATED coordinates, as the reference's Python layer
 *                                                         builds them (internals/geoseries.py:86-113); 0 - 3 list levels, "+l" or "+L"
 *   [List<]* FixedSizeList<f64, 2>                        native GeoArrow, interleaved
 * Sliced arrays (offset != 0 at any level), 64-bit list offsets (narrowed after a range check) and validity bitmaps with a bit
 * offset are handled.  One and two list levels are two geometry types each: `geom_type_hint` (GPK_GEOM_*, or -1) or the schema's
 * ARROW:extension:name (geoarrow.multipoint / geoarrow.multilinestring) picks MULTIPOINT / MULTILINESTRING, else LINESTRING / POLYGON.
 * *out_geom_type (may be NULL) = the handle's type.  Anything else: GPK_ERR_MISMATCHED_GEOMETRY. */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
    const char* format;
    const char* name;
    const char* metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema** children;
    struct ArrowSchema* dictionary;
    void (*release)(struct ArrowSchema*);
    void* private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void** buffers;
    struct ArrowArray** children;
    struct ArrowArray* dictionary;
    void (*release)(struct ArrowArray*);
    void* private_data;
};
#endif
int32_t gpk_geoarray_from_arrow(const struct ArrowArray* array, const struct ArrowSchema* schema, int32_t geom_type_hint,
                                void* stream, gpk_geoarray** out, int32_t* out_geom_type);
/* ... and the way back (py-geopolars/src/ffi.rs:35-52: `to_py_array` hands every result to Python as an ArrowArray / ArrowSchema pair
 * that the importer releases): the handle's column in HOST memory behind the two caller-provided structs, every buffer owned by the
 * library until the importer calls the structs' `release` callbacks (which free the buffers, the children and the private data; a
 * struct whose release is NULL has been released).  `layout`:
 *   GPK_ARROW_WKB          Binary ("z", i32 offsets) of ISO WKB, encoded on the GPU (gpk_geoarray_to_wkb) — how the reference holds
 *                          geometry columns (util.rs:11-24); ARROW:extension:name geoarrow.wkb
 *   GPK_ARROW_STRUCT       native GeoArrow, 0 - 3 "+l" levels by geometry type over Struct<x: f64, y: f64> — what the reference's Python
 *                          layer builds (internals/geoseries.py:86-113)
 *   GPK_ARROW_INTERLEAVED  the same nesting over FixedSizeList<f64, 2>
 * Native layouts carry ARROW:extension:name geoarrow.point / linestring / polygon / multipoint / multilinestring / multipolygon, so
 * that gpk_geoarray_from_arrow(to_arrow(x)) == x for every type.  Null rows keep their (empty) slots; the outermost array carries the
 * validity bitmap and null_count. */
#define GPK_ARROW_WKB 0
#define GPK_ARROW_INTERLEAVED 1
#define GPK_ARROW_STRUCT 2
int32_t gpk_geoarray_to_arrow(const gpk_geoarray* a, int32_t layout, void* stream, struct ArrowArray* out_array, struct ArrowSchema* out_schema);
/* Device -> host copy of a handle's GeoArrow buffers.  sizes[4] = {n_coords, n_parts, n_rings, n_geoms} is always
 * filled; NULL buffers are skipped (call once with NULLs to size the buffers). */
int32_t gpk_geoarray_download(const gpk_geoarray* a, int64_t sizes[4], double* xy, int32_t* geom_offsets,
                              int32_t* part_offsets, int32_t* ring_offsets, void* stream);

/* The Arrow validity bitmap of a handle, device -> host: *out_has_validity = 0 when every row is valid (nothing is
 * written); out_bitmap[(n_geoms + 7) / 8] may be NULL to ask only that. */
int32_t gpk_geoarray_validity(const gpk_geoarray* a, uint8_t* out_bitmap, int32_t* out_has_validity, void* stream);

/* ---- unary operators: GeoSeries::{area, centroid, envelope/bounds, affine_transform, ...} --- */
/* out arrays live in `out_space`; sizes are in elements.                                      */
/* area: geoseries.rs:14-16,188-190.  out[n_geoms] */
int32_t gpk_area(const gpk_geoarray* a, double* out, int32_t out_space, void* stream);
/* signed area (exterior orientation sign), same layout */
int32_t gpk_signed_area(const gpk_geoarray* a, double* out, int32_t out_space, void* stream);
/* centroid: geoseries.rs:18-21,192-194.  out_xy[2*n_geoms]; out_valid[n_geoms] bytes (0 = empty geometry -> null) */
int32_t gpk_centroid(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, int32_t out_space,
                     void* stream);
/* representative_point (GeoPandas representative_point, shapely point_on_surface; the rules of GEOS's InteriorPointArea /
 * InteriorPointLine / InteriorPointPoint): one point per row that lies in the row's geometry, where the centroid of an L shape, a
 * ring shape, a multipolygon or a polyline often does not.  out_xy[2*n_geoms]; out_valid[n_geoms] bytes (may be NULL);
 * out_width[n_geoms] (may be NULL).  Both coordinate layouts of gpk_geoarray_upload are accepted.
 *   POLYGON | MULTIPOLYGON, for every non-empty member (a member without rings or with an empty shell is ignored):
 *     scan line   centreY = (miny + maxy) / 2 of the member's coordinates (all rings).  loY = miny, hiY = maxy; for every coordinate
 *                 y of every ring: y <= centreY and y > loY sets loY = y, y > centreY and y < hiY sets hiY = y.
 *                 scanY = (loY + hiY) / 2: comparisons and one average, bit-exact.
 *     crossings   every ring edge (p0, p1) that is not horizontal and has min(y0, y1) <= scanY <= max(y0, y1), but not an edge
 *                 that meets the line only at its upper end (y0 == scanY && y1 < scanY, or y1 == scanY && y0 < scanY; this can
 *                 arise only when loY and hiY are adjacent doubles).  x = x0 when x0 == x1, else
 *                 x0 + (scanY - y0) * ((x1 - x0) / (y1 - y0)), every operation rounded on its own (no contraction).
 *     sections    the member's crossings in ascending order of x, ties broken by edge index, pair up: (0, 1), (2, 3), ...;
 *                 width = x[2k + 1] - x[2k].
 *     choice      the point is ((x[2k] + x[2k + 1]) / 2, scanY) of the widest section over all members;
 *                 a later section only when strictly wider: the first of equal widths wins in storage order.  out_width = that width.
 *     degenerate  a row without a section of positive width (zero area, all crossings coincident, an odd crossing count of invalid
 *                 input) answers its first coordinate with out_width exactly 0.
 *     invalid polygons: the value is unspecified, the call terminates
 *                 (gpk_validity says which rows are valid).
 *   Guarantee: the point of a valid polygon with out_width > 0 is strictly inside it as far as f64 carries: x is within
 *   1e-9 * (row box diagonal) + 4 ulp(max |x| of the row) of the exact midpoint of a section whose exact width is within that
 *   bound of the exact maximum, y is scanY bit for bit; a row whose widest section is at least 1e-6 * diagonal wide satisfies
 *   gpk_predicate_rowwise(contains) with its point.
 *   LINESTRING | MULTILINESTRING: among the interior vertices (coordinates that are neither first nor last of their member) the one
 *     nearest to the row's centroid (length-weighted: what gpk_centroid returns); a row without an interior vertex answers the
 *     nearest member end point.  Distance dx*dx + dy*dy in f64; a later vertex only when strictly nearer.  The answer is a
 *     coordinate of the row, bit for bit.  The centroid of a row without a member of positive length is geo's: the mean of the
 *     members' first coordinates, each weighted by its number of segments (a member of one coordinate: 1).
 *   POINT | MULTIPOINT: the member nearest to the mean of the members, same tie rule.  A POINT answers itself.
 *   Lineal and puntal rows give out_width = NaN.
 *   A null row, a row without a coordinate and a row with a NaN or infinite coordinate give out_valid = 0, a NaN point and
 *   out_width = NaN.  Empty members are ignored.
 * Errors and out_space as for gpk_centroid. */
int32_t gpk_representative_point(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, double* out_width, int32_t out_space, void* stream);
/* bounds (north-star) / envelope (geoseries.rs:28-33,200-202): out[4*n_geoms] = minx,miny,maxx,maxy;
 * empty geometry -> NaN x4 */
int32_t gpk_bounds(const gpk_geoarray* a, double* out4, int32_t out_space, void* stream);
/* euclidean_length: geoseries.rs:35-41.  out[n_geoms] */
int32_t gpk_euclidean_length(const gpk_geoarray* a, double* out, int32_t out_space, void* stream);
/* affine_transform: geoseries.rs:11-12,184-186.  m = [a, b, xoff, d, e, yoff] (upstream
 * `AffineTransform::from([f64;6])` order, which py-geopolars/src/geo.rs:10-16 passes through; the
 * Python docstring georust/geoseries.py:33 says [a,b,d,e,xoff,yoff] — that docstring is wrong).
 * out_xy[2*n_coords]; offsets are unchanged and shared with the input. */
int32_t gpk_affine_transform(const gpk_geoarray* a, const double m[6], double* out_xy,
                             int32_t out_space, void* stream);
/* rotate / scale / skew about a per-geometry origin (geoseries.rs:85-139,163-174; TransformOrigin of
 * py-geopolars/src/utils.rs:5-27 = centroid | bbox center | point) reduce to one affine matrix PER ROW:
 * matrices[6*n_geoms] in the same [a, b, xoff, d, e, yoff] order, living in `out_space`. */
int32_t gpk_affine_transform_rows(const gpk_geoarray* a, const double* matrices, double* out_xy,
                                  int32_t out_space, void* stream);
/* rotate / scale / skew about a per-geometry origin in ONE call (geoseries.rs:85-93,95-107,118-139): the origins
 * (TransformOrigin of py-geopolars/src/utils.rs:5-27: centroid | centre of the bounding box | a point) and the per-row
 * matrices are computed on the device, then applied like gpk_affine_transform_rows.
 *   kind    GPK_AFFINE_ROTATE  p0 = angle in degrees, counter-clockwise                      [c, -s, ox - c ox + s oy, s, c, oy - s ox - c oy]
 *           GPK_AFFINE_SCALE   p0 = xfact, p1 = yfact                                        [xf, 0, ox (1 - xf), 0, yf, oy (1 - yf)]
 *           GPK_AFFINE_SKEW    p0 = xs, p1 = ys in degrees (matrix of geoseries.rs:129-138)   [1, tan xs, -oy tan xs, tan ys, 1, -ox tan ys]
 *   origin  GPK_ORIGIN_CENTROID | GPK_ORIGIN_CENTER | GPK_ORIGIN_POINT (ox, oy)
 * out_xy[2*n_coords]; offsets are unchanged and shared with the input. */
#define GPK_AFFINE_ROTATE 0
#define GPK_AFFINE_SCALE  1
#define GPK_AFFINE_SKEW   2
#define GPK_ORIGIN_CENTROID 0
#define GPK_ORIGIN_CENTER   1
#define GPK_ORIGIN_POINT    2
int32_t gpk_affine_about_origin(const gpk_geoarray* a, int32_t kind, double p0, double p1, int32_t origin,
                                double ox, double oy, double* out_xy, int32_t out_space, void* stream);
/* reproject: analytic CRS reprojection of every coordinate (the closed-form part of geoseries.rs:148-151 `to_crs`; the general
 * PROJ path — arbitrary CRS strings, datum shifts, grids — stays with the reference).  All systems are on the WGS84
 * ellipsoid and are named by EPSG code:
 *   4326          geographic, x = lon, y = lat in degrees (the order proj_known_crs hands the reference)
 *   3857          spherical Web Mercator          3395  ellipsoidal Mercator
 *   32601-32660   UTM north, 32701-32760 UTM south (transverse Mercator, Krueger series to n^6)
 * Every ordered pair is one kernel launch; same -> same is a copy.  A coordinate FAILS — it is written as (NaN, NaN) and
 * counted — when an input is non-finite, a geographic latitude is beyond +-90, a transverse-Mercator destination is 90
 * degrees or more from its central meridian, or a result is non-finite (a Mercator at a pole).  Longitudes come out in
 * [-180, 180].  Accuracy is pinned within 12 degrees of the central meridian (1e-7 m); beyond, the series value is returned
 * as it is.  out_xy[2*n_coords]; offsets are unchanged and shared with the input.  n_failed (host) may be NULL: then
 * nothing is read back and, with a device output, the call does not wait for the stream.
 * An unsupported code: GPK_ERR_INVALID_ARGUMENT, message naming it, before any device work. */
int32_t gpk_crs_supported(int32_t epsg); /* 1 / 0; needs no device */
int32_t gpk_reproject(const gpk_geoarray* a, int32_t src_epsg, int32_t dst_epsg, double* out_xy, int64_t* n_failed,
                      int32_t out_space, void* stream);
/* envelope as a geometry (geoseries.rs:28-33; geo BoundingRect -> Rect::to_polygon): one closed 5-coordinate rectangle
 * per row (minx miny, maxx miny, maxx maxy, minx maxy, minx miny) — a POLYGON column whose ring_offsets are 5 i.
 * out_xy[10*n_geoms]; out_valid[n_geoms] bytes (0 = null or empty row: its rectangle is NaN).  The envelope of a point is
 * the point: POINT columns are reported (GPK_ERR_MISMATCHED_GEOMETRY), pass them through unchanged. */
int32_t gpk_envelope(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, int32_t out_space, void* stream);
/* exterior (geoseries.rs:43-47): the outer ring of each polygon as a LINESTRING column.  POLYGON columns only
 * (GeopolarsError::MismatchedGeometry otherwise).  out_geom_offsets[n_geoms+1]; out_xy capacity 2*n_coords(a) doubles
 * (NULL = size query); *n_out_coords = coordinates written.  Null rows give empty linestrings. */
int32_t gpk_exterior(const gpk_geoarray* a, double* out_xy, int32_t* out_geom_offsets, int64_t* n_out_coords,
                     int32_t out_space, void* stream);
/* explode (geoseries.rs:49-50; benches/explode.rs:10-24): one row per member of a multi-part geometry.  Pure offset
 * surgery — MULTIPOINT -> POINT, MULTILINESTRING -> LINESTRING, MULTIPOLYGON -> POLYGON, single-part columns explode to
 * themselves — so *out is a VIEW of `a` (coordinates and inner offsets are shared: `a` must outlive it; free it with
 * gpk_geoarray_free).  Members of a null row are null.  out_parent (optional, n_members i32 in `parent_space`): the row
 * each member came from — the index a dataframe repeats its other columns by. */
int32_t gpk_explode(const gpk_geoarray* a, int32_t* out_parent, int32_t parent_space, void* stream, gpk_geoarray** out);
/* rows of a handle (n_geoms) — e.g. of an exploded view */
int32_t gpk_geoarray_len(const gpk_geoarray* a, int64_t* out_n);
/* geom_type (geoseries.rs:60-73): the column's pygeos type id per row, -1 for null rows.  out[n_geoms] i8 */
int32_t gpk_geom_type(const gpk_geoarray* a, int8_t* out, int32_t out_space, void* stream);
/* is_empty (geoseries.rs:75-76; geo HasDimensions::is_empty): out[n_geoms] bytes 0/1, 0 for null rows */
int32_t gpk_is_empty(const gpk_geoarray* a, uint8_t* out, int32_t out_space, void* stream);
/* is_ring (geoseries.rs:78-83; geo-types LineString::is_closed: first == last, an empty linestring counts as closed).
 * LINESTRING columns only.  out[n_geoms] bytes 0/1, 0 for null rows */
int32_t gpk_is_ring(const gpk_geoarray* a, uint8_t* out, int32_t out_space, void* stream);
/* x / y (geoseries.rs:177-180): POINT columns only; either output may be NULL; NaN for null rows */
int32_t gpk_point_xy(const gpk_geoarray* a, double* out_x, double* out_y, int32_t out_space, void* stream);
/* geodesic_length (geoseries.rs:52-58,216-218; methods of py-geopolars/src/geo.rs:61-78): metres along the ellipsoid /
 * sphere, coordinates = (lon, lat) degrees; linestrings = their segments, polygons = exterior rings only, points = 0
 * (the row rule of euclidean_length).  out[n_geoms]; null rows NaN.
 *   GPK_GEODESIC_HAVERSINE  geo 0.27 HaversineLength: great circle on the mean-radius sphere (6371008.8 m)
 *   GPK_GEODESIC_VINCENTY   geo 0.27 VincentyLength: Vincenty's inverse formula on WGS84; a row holding a segment upstream
 *                           answers with Err(FailedToConverge) (nearly antipodal end points) is NaN
 *   GPK_GEODESIC_KARNEY     "geodesic", the Python default: geo 0.27 GeodesicLength = Karney's algorithm (J. Geodesy 87, 2013,
 *                           through geographiclib-rs) on WGS84 — order-6 series, Newton's method with bisection fallback */
#define GPK_GEODESIC_KARNEY    0
#define GPK_GEODESIC_HAVERSINE 1
#define GPK_GEODESIC_VINCENTY  2
int32_t gpk_geodesic_length(const gpk_geoarray* a, int32_t method, double* out, int32_t out_space, void* stream);
/* Geodesic area and perimeter on WGS84 (geo's GeodesicArea: geodesic_area_signed / geodesic_area_unsigned / geodesic_perimeter; Karney's
 * order-6 area series, csrc/gpk_geodesic.h).  Coordinates are (lon, lat) in degrees; an EDGE is the shortest geodesic between
 * consecutive ring coordinates as stored (rings are closed in storage; nothing is closed for the caller).
 *   - A ring's signed area is the area to the LEFT of its direction of travel, reduced to (-A0/2, A0/2], A0 = 510065621724088.5 m^2 the
 *     area of the ellipsoid: counter-clockwise rings are positive.  The reduction uses the ring's summed prime-meridian transit count
 *     (an odd count adds -+A0/2), so rings around a pole and rings across the antimeridian come out right.
 *   - GPK_GEODESIC_AREA_SIGNED: out_area[row] = the sum of the signed areas of ALL its rings as stored; holes wound opposite to their
 *     shells subtract themselves.
 *   - without the flag: out_area[row] = sum over parts of (|shell| - sum |hole|), the shell being a part's first ring.  A ring that
 *     covers MORE THAN HALF the ellipsoid therefore reports its complement: |.| of a value reduced to (-A0/2, A0/2].
 *   - out_perimeter[row] = the length in metres of every ring of every part, HOLES INCLUDED — not the exterior-only rule of
 *     gpk_geodesic_length.
 *   - LINESTRING / MULTILINESTRING / POINT / MULTIPOINT columns give 0 for both; null rows give NaN; a row holding a latitude outside
 *     [-90, 90] or a NaN coordinate gives NaN.
 * out_area[n_geoms], out_perimeter[n_geoms] in out_space; either may be NULL (neither: nothing is done).
 * Unknown flag bits: GPK_ERR_INVALID_ARGUMENT before any device work.  Sums are error-free pairs in a fixed order, without
 * floating-point atomics: the same bits from run to run.  Stream-ordered (host outputs are copied on the stream and waited for). */
#define GPK_GEODESIC_AREA_SIGNED 1u
int32_t gpk_geodesic_area(const gpk_geoarray* a, uint32_t flags, double* out_area, double* out_perimeter, int32_t out_space,
                          void* stream);
/* The inverse geodesic problem row by row (geo's GeodesicDistance and GeodesicBearing): a and b are POINT columns of (lon, lat) degrees.
 *   out_s12[i]   metres between a[i] and b[b_rows ? b_rows[i] : i] along the WGS84 ellipsoid
 *   out_azi1[i]  forward azimuth at a[i], degrees clockwise from north in [-180, 180]
 *   out_azi2[i]  forward azimuth at the b point (the direction of arrival carried on), same convention
 * Any output may be NULL.  `b_rows` (same space as the outputs) follows gpk_distance_rowwise: NULL = identity (the row counts must then
 * match, else GPK_ERR_INVALID_ARGUMENT); an entry >= n_geoms(b), a null or empty row on either side, a NaN coordinate or a latitude
 * outside [-90, 90] gives NaN.  Any other family: GPK_ERR_MISMATCHED_GEOMETRY.  Both refusals come before any device work. */
int32_t gpk_geodesic_inverse(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double* out_s12, double* out_azi1,
                             double* out_azi2, int32_t out_space, void* stream);
/* The direct geodesic problem row by row (geo's GeodesicDestination): from the POINT a[i] along azimuth azi1 (degrees clockwise from
 * north) for s12 metres (negative: backwards).  n_azi and n_s12 are each 1 (one value for every row, not expanded) or n_geoms(a), else
 * GPK_ERR_INVALID_ARGUMENT; azi1 and s12 live in out_space.  out_xy[2 * n_geoms] interleaved (lon in [-180, 180], lat); out_azi2
 * (may be NULL) the forward azimuth at the destination.  Null or empty rows, NaN or infinite inputs and latitudes outside [-90, 90]
 * give NaN.  Any other family: GPK_ERR_MISMATCHED_GEOMETRY.  Both refusals come before any device work. */
int32_t gpk_geodesic_direct(const gpk_geoarray* a, const double* azi1, int64_t n_azi, const double* s12, int64_t n_s12, double* out_xy,
                            double* out_azi2, int32_t out_space, void* stream);
/* simplify (geoseries.rs:108-116,240-242): Ramer-Douglas-Peucker as geo 0.27 runs it (algorithm/simplify.rs): per
 * coordinate sequence (linestring / ring), the farthest point from the chord decides (the LAST one among equals), a
 * range whose farthest point is within `epsilon` loses its interior unless the sequence would drop below 2 (linestrings)
 * / 4 (polygon rings) coordinates; end points are always kept; epsilon <= 0 returns the input.  The nesting above the
 * sequences does not change: the result has the input's geom / part offsets and
 *   out_seq_offsets[n_seq + 1]   the new innermost offsets (ring_offsets, or geom_offsets of a LINESTRING column)
 *   out_xy                       capacity 2 * n_coords(a) doubles (NULL = size query); *n_out_coords = coordinates kept.
 * LINESTRING / MULTILINESTRING / POLYGON / MULTIPOLYGON columns (points: GPK_ERR_MISMATCHED_GEOMETRY, pass through). */
int32_t gpk_simplify(const gpk_geoarray* a, double epsilon, double* out_xy, int32_t* out_seq_offsets,
                     int64_t* n_out_coords, int32_t out_space, void* stream);
/* convex_hull: geoseries.rs:23-26,196-198.  Output = POLYGON array, one closed CCW ring per geometry.
 * out_ring_offsets[n_geoms+1]; out_xy capacity must be >= 2*(n_coords + n_geoms) doubles. */
int32_t gpk_convex_hull(const gpk_geoarray* a, double* out_xy, int32_t* out_ring_offsets,
                        int32_t out_space, void* stream);
/* minimum_rotated_rectangle (GeoPandas minimum_rotated_rectangle, shapely oriented_envelope) and minimum_bounding_circle /
 * minimum_bounding_radius: the two bounding shapes of a row's convex hull.  All six geometry families; a row is its set of
 * coordinates (holes and members only contribute points, as in gpk_convex_hull).  Both coordinate layouts of gpk_geoarray_upload are
 * accepted.  Both outputs have a fixed size per row:
 *   gpk_minimum_rotated_rectangle   out_xy[n_geoms * 5 * 2]: the closed ring c0 c1 c2 c3 c0; out_valid[n_geoms] bytes (may be NULL)
 *   gpk_minimum_bounding_circle     out_center_xy[n_geoms * 2] (may be NULL), out_radius[n_geoms], out_valid[n_geoms] (may be NULL)
 * A null row, a row without a coordinate and a row with a NaN or infinite coordinate give out_valid = 0 and NaN in every output slot
 * (the rule of gpk_representative_point).
 * Let v_0 .. v_{h-1} be the hull ring exactly as gpk_convex_hull writes it: counter-clockwise, starting at the lexicographically
 * smallest vertex, no collinear vertices, closing vertex dropped.
 *   Rectangle.  For edge i, with a = v_i and d = v_{i+1} - a: L2 = d . d; for every hull vertex w, with u = w - a taken first,
 *     s = u . d and t = d x u; smin, smax and tmax are taken over the hull (smin <= 0 <= smax and tmax >= 0 because a is among the
 *     vertices); A_i = (smax - smin) * tmax.  The rectangle on edge i has area A_i / L2_i.
 *     choice      the edge of least area, areas compared by cross-multiplication: A_i * L2_j < A_j * L2_i.  A later edge wins only when
 *                 strictly smaller: equal areas on exactly representable data go to the lowest edge index.
 *     corners     c0 = a + (smin / L2) d, c1 = a + (smax / L2) d, c2 = c1 + (tmax / L2) (-d_y, d_x), c3 = c0 + (tmax / L2) (-d_y, d_x).
 *                 The output is c0 c1 c2 c3 c0: counter-clockwise, the fifth coordinate is the first bit for bit.
 *     degenerate  one distinct point: that point five times.  All coordinates collinear (hull ring p q p): p q q p p.  Both are valid rows.
 *     Every operation is rounded on its own (no contraction).  Guarantee: the corners are within 1e-9 * (row box diagonal) +
 *     4 ulp(max |coordinate| of the row) of the exact rectangle on some edge whose exact area is within that bound (times the
 *     perimeter) of the exact minimum.
 *   Circle.  The unique smallest circle that contains the row's coordinates, computed in row-local coordinates with origin v_0.
 *     A two-point support has its midpoint as centre; a three-point support uses the circumcentre formula on differences from the
 *     first support point; the radius is the square root of the squared distance from the centre to a support point.  One distinct
 *     point gives radius exactly 0 and centre = the point.  Method: farthest-point iteration from v_0 and the vertex farthest from it
 *     (csrc/gpk_minbound.h states every step); it runs at most MBG_CIRCLE_ITERS times, and if it ever stops there the answer is the
 *     current centre with the distance to the farthest vertex as radius: a circle that still contains the row.  Guarantee: centre and
 *     radius within the bound above of the exact ones.
 * Every data-dependent loop carries a bound derived from h: no input can keep a wave spinning.
 * Errors: GPK_ERR_INVALID_ARGUMENT ("NULL argument") for a NULL a, out_xy or out_radius, before any device work; out_space as for
 * gpk_centroid. */
#define MBG_CIRCLE_ITERS 64
int32_t gpk_minimum_rotated_rectangle(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, int32_t out_space, void* stream);
int32_t gpk_minimum_bounding_circle(const gpk_geoarray* a, double* out_center_xy, double* out_radius, uint8_t* out_valid, int32_t out_space,
                                    void* stream);

/* ---- row-wise binary operators ------------------------------------------------------------ */
/* distance: geoseries.rs:141-146,248-251 ("1-to-1 row-wise").  `b_rows` (optional, same space as
 * out) maps row i of `a` to row b_rows[i] of `b` — the take() a caller would otherwise materialise;
 * NULL = identity (then n_geoms must match); an entry >= n_geoms(b) behaves like a null row of b
 * (distance NaN, predicate false — the out-of-range rule of gpk_take_*).  out[n_geoms(a)].  Supported: every pair of POINT,
 * MULTIPOINT, LINESTRING, MULTILINESTRING, POLYGON and MULTIPOLYGON.
 * Pairs with a POINT column: the point kernels (geo's EuclideanDistance per family; b_rows needs the POINT array on the left).
 * Pairs of two non-point columns (gpk_pairdist.hip), for A = a[i], B = b[b_rows[i]]:
 *   - a null or EMPTY side gives NaN; empty = no member has a coordinate (empty members of a multi-geometry are ignored).
 *     NaN is what shapely 2 / GeoPandas return; geo 0.27 panics or returns f64::MAX there [verify: recalled, not checked];
 *   - 0.0 exactly when A and B intersect as closed point sets, decided with exact orientations (a segment of A meets a segment
 *     of B, touching and collinear overlap included, or a vertex of one side is inside or on a polygonal other side; holes
 *     excluded).  A disjoint pair is never 0: a vertex one ulp off a segment gives a tiny positive distance;
 *   - otherwise the minimum over every vertex of one side and every segment of the other, both ways, of the point-segment
 *     distance, compared exactly as fractions, one square root at the end.  A one-coordinate sequence and every MULTIPOINT
 *     member is a degenerate segment; every ring of a polygon counts.  For disjoint sets this is the set distance, within
 *     16 u (d + 2 lmax) of the exact value (lmax: the longest segment of the pair).
 *   distance(a, b) and distance(b, a) evaluate the same pairs in the same order.  Device outputs are stream-ordered (rows above
 *   the large-row threshold are finished by a second launch on the same stream, without a read-back). */
int32_t gpk_distance_rowwise(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows,
                             double* out, int32_t out_space, void* stream);
/* Magnitude range of gpk_distance_rowwise and gpk_nearest_join.  The kernels compare squared point-segment distances as
 * fractions by cross-multiplication (gpk_distance.h segment_dist2 / frac_less): the products grow as the sixth power of the
 * coordinate differences.  Measured on MI355X by scaling georeferenced columns (Web Mercator coordinates ~2^24, features of
 * 0.5 - 50 m, points from 1 ulp to 3 m off an edge) by 2^k: both return exactly 2^k times the unscaled answer (and the same
 * pairs) for |k| <= 166 and depart at |k| = 168, i.e. at coordinates near 2^192 (6e57) or 2^-144 (5e-44).  Supported:
 * coordinates and coordinate differences within 2^-120 .. 2^120 (1e-36 .. 1e36) in magnitude; tests/test_gpu_georeferenced.py
 * holds |k| <= 100 of the same columns to exact scaling.  The non-point pairs use the same fraction comparison (products of the
 * sixth power of coordinate differences) and are held to exact 2^k scaling for |k| <= 100 by tests/test_gpu_distance_pairs.py
 * (hand-made cases, also at UTM and Web Mercator placements, and random columns); beyond that they were not measured. */
/* A row map that is used more than once (a dataframe's foreign-key column joined against the same geometry column for
 * every batch of points) can be prepared ONCE: gpk_rowmap_build orders the left rows by target (targets by descending
 * vertex count, so that the 64 rows one wave takes walk equally long linestrings) and keeps the order in HBM;
 * gpk_distance_rowmap then runs the distance kernel alone, stream-ordered.  LINESTRING right sides (the grouped schedule);
 * gpk_distance_rowwise with b_rows builds, uses and drops such a map internally when a target has 8 or more rows on
 * average.  b_rows in `rows_space`; the build synchronises the stream. */
typedef struct gpk_rowmap gpk_rowmap;
int32_t gpk_rowmap_build(const gpk_geoarray* b, const uint32_t* b_rows, int64_t n_rows, int32_t rows_space,
                         void* stream, gpk_rowmap** out);
int32_t gpk_rowmap_free(gpk_rowmap* map);
int32_t gpk_rowmap_nbytes(const gpk_rowmap* map, int64_t* out_bytes);
/* out[n_geoms(a)] as gpk_distance_rowwise(a, b, b_rows, ...) would fill it; a POINT, b the LINESTRING array of the map */
int32_t gpk_distance_rowmap(const gpk_geoarray* a, const gpk_geoarray* b, const gpk_rowmap* map, double* out,
                            int32_t out_space, void* stream);
/* Discrete Hausdorff and discrete Frechet distance, row-wise: GeoPandas' GeoSeries.hausdorff_distance(other, densify) and
 * GeoSeries.frechet_distance(other, densify) (GEOS DiscreteHausdorffDistance / DiscreteFrechetDistance).  `b_rows`, out[n_geoms(a)],
 * `out_space`, stream ordering and the out-of-range rule are those of gpk_distance_rowwise (b_rows works for every pair of
 * families here).
 * Samples.  A row is its coordinate sequences: a LINESTRING is one sequence; every ring of a POLYGON or MULTIPOLYGON and every
 * linestring of a MULTILINESTRING is a sequence; every MULTIPOINT member and a POINT is a sequence of one coordinate.  Polygon
 * interiors play no part: both measures are between boundaries, as in GEOS.  With subdivisions = k >= 1 the samples of a sequence
 * p_0 .. p_(n-1) are, for every segment (p_i, p_(i+1)) and j = 0 .. k-1, the doubles
 *     x = p_i.x + (double)j * ((p_(i+1).x - p_i.x) / (double)k)      and the same for y,
 * every operation rounded on its own (no contraction), followed by the last vertex as itself; k = 1 means the vertices.  These
 * doubles are part of the contract.  Sample counts and costs are computed in 64 bits.  k outside 1 .. GPK_MAX_SUBDIVISIONS is
 * GPK_ERR_INVALID_ARGUMENT before any device work (GeoPandas' densify fraction f maps to k = rint(1 / f)).
 *
 * gpk_hausdorff_distance: every pair of the six families, POINT included.  H = max(h(A->B), h(B->A)); h(A->B) is the maximum over
 * the samples of A of the minimum over the segments of B (undensified) of the point-segment distance.  Segments as in
 * gpk_distance_rowwise: coordinate c gives (c, c + 1) inside its sequence, else the degenerate (c, c).
 *   - terms are squared point-segment distances kept as fractions (pair_seg_dist2, csrc/gpk_pairdist.h) and compared by
 *     cross-multiplication; one square root is taken at the end;
 *   - there is no substitution for a computed zero: two identical rows give exactly 0.0;
 *   - a null side, an empty side (no member has a coordinate; a POINT with a NaN coordinate) or a b_rows entry out of range
 *     gives NaN.
 *   Accuracy: within 16 u (H + 2 lmax) of the exact value over the contract's samples, lmax the longest undensified segment of the
 *   pair — the bound gpk_distance_rowwise states: every term carries it, and a max of mins moves by no more than its worst term.
 *   hausdorff(a, b) and hausdorff(b, a) evaluate the same terms in the same order (the columns are taken in canonical order, the
 *   final choice between the two directed values does not look at their order): they are bit-identical, as are two calls on the
 *   same input.  Magnitude range: as gpk_distance_rowwise.
 *
 * gpk_frechet_distance: LINESTRING x LINESTRING only; any other pair is GPK_ERR_MISMATCHED_GEOMETRY, because the measure is defined
 * on ONE ordered sequence per side (GEOS flattens a multi-geometry into one sequence, which measures the jumps between its members;
 * that is not offered).  The discrete Frechet distance of the two sample sequences P (n' samples) and Q (m' samples):
 *     c(0,0) = d(0,0);  c(i,j) = max(d(i,j), min(c(i-1,j), c(i,j-1), c(i-1,j-1))), missing neighbours left out;
 *     result = sqrt(c(n'-1, m'-1)),
 * on squared distances d = dx*dx + dy*dy in f64.  A one-coordinate linestring is a sequence of one sample.  A null or empty side
 * or a b_rows entry out of range gives NaN.
 *   Accuracy: relative error at most 4 u — each difference is correctly rounded (u), the two squares and the sum add three more
 *   roundings, so every d is within a factor 1 +- 4u; max and min are monotone; the square root halves the error and adds u.  The
 *   result is exactly 0 iff the exact value is 0.  frechet(a, b) and frechet(b, a) are bit-identical (max and min only select).
 *   Rows whose SHORTER side has more than GPK_FRECHET_MAX_SHORT samples after densification are not computed: the result is NaN
 *   and the row is counted in *n_over.  16384 samples are a boundary column of 128 KB in the 160 KB of LDS behind a row
 *   (csrc/gpk_frechet.h).  n_over (host) may be NULL: then nothing is read back and a device output stays stream-ordered; with
 *   n_over the call waits for the stream, as gpk_reproject does for n_failed. */
#define GPK_FRECHET_MAX_SHORT 16384
#define GPK_MAX_SUBDIVISIONS 4096
int32_t gpk_hausdorff_distance(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, int32_t subdivisions,
                               double* out, int32_t out_space, void* stream);
int32_t gpk_frechet_distance(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, int32_t subdivisions,
                             double* out, int64_t* n_over, int32_t out_space, void* stream);
/* contains / within / intersects row-wise (north-star additions to the trait; semantics from the
 * dispatch table spatial_index.rs:89-137, geo 0.27 traits).  out[n] bytes 0/1.  Pairs with an answer:
 * point x polygonal (all three), polygonal x polygonal (intersects; contains / within = "the contained side
 * is not empty and a subset of the other", every member of a multipolygon counted), lineal contains point /
 * point within lineal, point x point (equality); any other pair is false. */
int32_t gpk_predicate_rowwise(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows,
                              int32_t predicate, uint8_t* out, int32_t out_space, void* stream);

/* ---- spatial index + join: spatial_index.rs:37-204,314-350 -------------------------------- */
/* SpatialIndex::try_from(&Series) (spatial_index.rs:320-334): bbox per geometry + a uniform-grid
 * directory over the bboxes (the GPU replacement for rstar's R-tree) + per-polygon edge slabs. */
int32_t gpk_index_build(const gpk_geoarray* a, void* stream, gpk_index** out);
/* The same with a choice of tables and, optionally, precomputed leaves:
 *   parts      GPK_INDEX_BBOX_GRID (always built: what rstar holds, the candidate generator of every join arm)
 *              | GPK_INDEX_PIP (point-in-polygon raster + edge slabs; only point x polygonal joins read them — a
 *                polygon x polygon join served by an index without them costs a fraction of the build).  A point join
 *                against an index built without GPK_INDEX_PIP still answers exactly, through the slow generic walk.
 *   bbox4_dev  NULL, or n_geoms x (minx, miny, maxx, maxy) in DEVICE memory (NaN x4 = empty geometry): the leaves
 *              another rank computed with gpk_bounds for its shard and all-gathered — the bounds
 *              pass over the coordinates is skipped.
 * gpk_index_build(a, ...) == gpk_index_build_ex(a, GPK_INDEX_BBOX_GRID | GPK_INDEX_PIP, NULL, ...). */
#define GPK_INDEX_BBOX_GRID 1
#define GPK_INDEX_PIP       2
#define GPK_INDEX_PIP_LIGHT 4 /* with GPK_INDEX_PIP: no per-entry level-2 records for cells where several parts meet — about half
                                 the build time on overlapping right sides for ~10 % slower point joins: what gpk_spatial_join builds
                                 for itself when it is handed no index (an index that serves one join) */
#define GPK_INDEX_PIP_FULL  8 /* with GPK_INDEX_PIP: those records ALWAYS.  By default a column of very many small parts (more than two per
                                 cell of the 2048 x 2048 raster: 5M power-law multipolygons) gets a 4096 x 4096 raster, plain entry lists
                                 and a box per part instead: 118 ms / 1.7 GB / 2.0 ms per 6.25M-point join against 215 ms / 2.7 GB / 1.6 ms
                                 with the records — worth it for an index that serves a few hundred joins */
int32_t gpk_index_build_ex(const gpk_geoarray* a, int32_t parts, const double* bbox4_dev, void* stream,
                           gpk_index** out);
int32_t gpk_index_free(gpk_index* idx);
/* A query on the index by itself — what the reference's own index tests do (spatial_index.rs:383-393,422-429):
 * `r_tree.locate_in_envelope(&AABB::from_corners(lo, hi))` = every leaf (one per indexed geometry: its bounding box) CONTAINED in the
 * query box, `locate_in_envelope_intersecting` = every leaf that meets it; both with closed intervals (a leaf touching the query box's
 * border is contained / intersecting — rstar AABB::contains_envelope / intersects).  Batched: n_boxes query boxes
 *   boxes4[4 * n_boxes]      two corners (x0, y0, x1, y1) per query, in `space`; ordered as AABB::from_corners orders them (component-wise
 *                            min / max); a box with a NaN matches nothing
 *   out_counts[n_boxes]      u32 leaves per query (may be NULL)
 *   out_pairs[2 * capacity]  u32 (query, geometry index) interleaved, sorted by (query, index) (NULL + capacity 0: count only)
 *   *n_pairs                 total, always set (GPK_ERR_CAPACITY when > capacity and pairs were asked for)
 * Null and empty geometries have no leaf.  No geometry is read: the answer comes from the index's boxes and grid directory. */
#define GPK_QUERY_CONTAINED    0 /* rstar RTree::locate_in_envelope */
#define GPK_QUERY_INTERSECTING 1 /* rstar RTree::locate_in_envelope_intersecting */
int32_t gpk_index_query_envelope(const gpk_index* idx, const double* boxes4, int64_t n_boxes, int32_t mode,
                                 uint32_t* out_counts, uint32_t* out_pairs, int64_t pair_capacity, int64_t* n_pairs,
                                 int32_t space, void* stream);
int32_t gpk_index_nbytes(const gpk_index* idx, int64_t* out_bytes);
/* What the index holds (tests and bench.py report it; nothing in a join depends on the caller knowing):
 *   out = {raster side R (0: no point-in-polygon tables), one-part-per-cell ("lean") 0/1, local chains 0/1 (`test` sub-cells
 *          decided from one or two ring edges in the owning lane), LDS routing image 0/1 (R <= 512), entry lists dominate 0/1 (overlapping parts,
 *          very many small parts: the general tile kernel runs one point per lane), cells of the routing image that name their
 *          polygon themselves ("own": strictly inside the owner part of their block of 8 x 4 cells), raster cells strictly inside one
 *          part (an index with a routing image counts them; the difference still reads its level-1 word), 0} */
int32_t gpk_index_describe(const gpk_index* idx, int64_t out[8]);

/*
 * spatial_join refine (spatial_index.rs:74-143): all (l, r) with predicate(left[l], right[r]) true,
 * emitted SORTED by (l, r) (rstar's traversal order is unspecified; the shim may compare sets).
 *   out_counts[n_left]   u32 hits per left row (may be NULL)
 *   out_pairs[2*cap]     u32 (l, r) interleaved (may be NULL when cap == 0: count-only mode)
 *   *n_pairs             total hits (always set; GPK_ERR_CAPACITY if > cap and pairs requested)
 * `right_index` may be NULL (built on the fly like spatial_index.rs:60-71).  The index such a call builds STAYS on the right-side
 * handle WHEN THE HANDLE OWNS ITS BUFFERS (host uploads, gpk_geoarray_from_wkb / _from_arrow, results of this library: nobody can
 * change those bytes, so the index cannot go stale) and is freed with it: the reference's default call shape —
 * SpatialJoinArgs::default() has r_index: None, spatial_index.rs:24-35 — repeated against the same series pays for one build.
 * A handle that BORROWS device buffers (GPK_MEM_DEVICE descriptors: the caller may rewrite them between calls) gets a fresh index
 * in every such call.  Only indexes of at most GPK_AUTO_INDEX_MAX_MB (environment, default 256) are kept; GPK_AUTO_INDEX=0 builds and
 * frees per call; gpk_geoarray_nbytes includes the kept indexes.
 * Geometry dispatch = the match of spatial_index.rs:89-137: point <-> polygon / multipolygon on either side
 * (`poly.contains(point)` whatever the predicate), polygonal x polygonal `intersects`, polygon / multipolygon x POLYGON
 * `contains` (:99-101,107-111; upstream's DE-9IM relate restated as "right is not empty and a subset of left"),
 * point <-> linestring / multilinestring on either side (`line.contains(point)`); every other combination (e.g. `contains`
 * with a multipolygon on the right, `within` for polygonal pairs) is upstream's `_ => false`: an empty result, not an error.
 * `left_row_base` is added to every emitted l (row-sharded multi-GPU runs).
 */
int32_t gpk_spatial_join(const gpk_geoarray* left, const gpk_geoarray* right,
                         const gpk_index* right_index, int32_t predicate, uint32_t left_row_base,
                         uint32_t* out_counts, uint32_t* out_pairs, int64_t pair_capacity,
                         int64_t* n_pairs, int32_t out_space, void* stream);

/*
 * Nearest-neighbour join (GeoPandas sjoin_nearest): for every left row l, every right row r whose distance equals the row's minimum
 * distance EXACTLY, in the kernel's own f64 arithmetic — ties are all returned.  Left: POINT.  Right: POINT, MULTIPOINT, LINESTRING,
 * MULTILINESTRING, POLYGON or MULTIPOLYGON (anything else: GPK_ERR_MISMATCHED_GEOMETRY).
 *   distance(l, r)       geo's Euclidean distance as gpk_distance_rowwise defines it (0 for a point inside or on a polygon); every
 *                        returned distance is bit for bit what gpk_distance_rowwise's per-row kernel returns for the pair (its grouped
 *                        schedule for LINESTRING right sides with >= 8 rows per target agrees within its 1e-9 contract)
 *   max_distance         only pairs with d <= max_distance (closed); INFINITY = no limit; negative or NaN: GPK_ERR_INVALID_ARGUMENT
 *   never matched        null or empty left rows, left points with a NaN coordinate: count 0
 *   never candidates     null and empty right rows (they have no leaf in the index) — unlike row-wise distance, which gives 0.0 for an
 *                        empty linestring.  An empty right side, or one of null / empty rows only, gives no pairs.
 *   out_counts[n_left]   u32 matches per left row (may be NULL)
 *   out_pairs[2*cap]     u32 (l, r) interleaved, sorted by (l, r) (NULL with cap == 0: count-only mode)
 *   out_dist[cap]        f64 distance of each pair (may be NULL)
 *   *n_pairs             total, always set; GPK_ERR_CAPACITY when > cap and pairs were asked for
 * Magnitude range: as gpk_distance_rowwise (exact for coordinates within 2^-120 .. 2^120).
 * `left_row_base` is added to every emitted l.  All buffers live in `out_space`.  `right_index`: an index of `right` carrying the bbox
 * grid (else GPK_ERR_INVALID_ARGUMENT), or NULL: a GPK_INDEX_BBOX_GRID index is built for the call and freed (it is not kept on the
 * handle).  Synchronous, like gpk_spatial_join.
 */
int32_t gpk_nearest_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double max_distance,
                         uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist, int64_t pair_capacity,
                         int64_t* n_pairs, int32_t out_space, void* stream);

/*
 * Nearest-neighbour join for any two geometry families (GeoPandas sjoin_nearest with lines or polygons on the left: buildings to the
 * nearest road, roads to the nearest station): for every left row l, every right row r with d(l, r) == min over the usable right rows
 * r' of d(l, r') and d(l, r) <= max_distance.  Left and right are each any of POINT, MULTIPOINT, LINESTRING, MULTILINESTRING, POLYGON,
 * MULTIPOLYGON — all 36 ordered pairs (anything else: GPK_ERR_MISMATCHED_GEOMETRY).  gpk_nearest_join is unchanged and keeps refusing
 * a non-POINT left side; the argument list, outputs, capacity rule and index rule here are its own.
 *   d(l, r)              the library's own row-wise distance of the pair, as in gpk_dwithin_join: the value the per-row kernel of
 *                        gpk_distance_rowwise(left, right, ...) computes for these two columns — the same device routine, the same
 *                        lane-group size, the same lane order, the work-group routine above PD_LARGE_COST — so every returned distance
 *                        is bit for bit what that call returns for the pair (0 for rows that meet, contained rows included).  (Its
 *                        grouped schedule for LINESTRING right sides with >= 8 rows per target agrees within its 1e-9 contract.)
 *   ties                 equality of those doubles; all rows at the minimum are returned
 *   max_distance         only pairs with d <= max_distance (closed); INFINITY = no limit; negative or NaN: GPK_ERR_INVALID_ARGUMENT
 *                        before any device work
 *   never matched,       null rows, EMPTY rows (no member has a coordinate) and POINT rows with a NaN coordinate, on either side (the
 *   never candidates     rule of gpk_dwithin_join): such a left row has count 0, such a right row is nobody's neighbour.  An empty right
 *                        side, or one of such rows only, gives no pairs.
 *   POINT left           counts, pairs and distances are byte for byte those of gpk_nearest_join (both evaluate
 *                        point_geom_distance<G, KIND> with G chosen from the right column)
 *   out_counts[n_left]   u32 matches per left row (may be NULL)
 *   out_pairs[2*cap]     u32 (l, r) interleaved, sorted by (l, r) (NULL with cap == 0: count-only mode)
 *   out_dist[cap]        f64 d(l, r) of each pair (may be NULL)
 *   *n_pairs             total, always set; GPK_ERR_CAPACITY when > cap and pairs were asked for.  More than 2^31 - 1 bbox candidates
 *                        (right boxes meeting a left box grown by the row's search radius: the distance to the right row whose box is
 *                        nearest, at most max_distance) or pairs: GPK_ERR_CAPACITY, shard the left side.
 * The result does not depend on scheduling: two calls give identical bytes.  `left_row_base` is added to every emitted l.  All buffers
 * live in `out_space`.  `right_index`: an index of `right` carrying the bbox grid (else GPK_ERR_INVALID_ARGUMENT), or NULL: a
 * GPK_INDEX_BBOX_GRID index is built for the call and freed (it is not kept on the handle).  Synchronous, like gpk_spatial_join.
 * Magnitude range: as gpk_distance_rowwise.
 */
int32_t gpk_nearest_join_any(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double max_distance,
                             uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist, int64_t pair_capacity,
                             int64_t* n_pairs, int32_t out_space, void* stream);

/*
 * k-nearest-neighbours join for any two geometry families (spatial weights over a column against itself, inverse-distance
 * interpolation, "the five nearest roads"): for every left row l, the k usable right rows nearest to it, nearest first.  Left and right
 * are each any of POINT, MULTIPOINT, LINESTRING, MULTILINESTRING, POLYGON, MULTIPOLYGON — all 36 ordered pairs (anything else:
 * GPK_ERR_MISMATCHED_GEOMETRY).
 *   d(l, r)              the library's own row-wise distance of the pair, as in gpk_nearest_join_any: the value the per-row kernel of
 *                        gpk_distance_rowwise(left, right, ...) computes for these two columns — the same device routine, the same
 *                        lane-group size, the same lane order, the work-group routine above PD_LARGE_COST — so every returned distance
 *                        is bit for bit what that call returns for the pair (0 for rows that meet, contained rows included; -0.0 is
 *                        returned as +0.0).  (Its grouped schedule for LINESTRING right sides with >= 8 rows per target agrees within
 *                        its 1e-9 contract.)
 *   key                  (bits(d), r), compared lexicographically.  Distances are non-negative, so the order of the bits is the order
 *                        of the values; the keys of a left row are distinct.
 *   result of a row      the min(k, m) smallest keys, m the number of usable right rows with d <= max_distance.  A tie at the k-th
 *                        place goes to the lower right row: exactly k pairs are returned when k exist — this is NOT the tie-inclusive
 *                        set of gpk_nearest_join_any (at k = 1 it is that set's lowest right row).
 *   k                    1 .. GPK_KNN_MAX_K (64), else GPK_ERR_INVALID_ARGUMENT.  The cap is a limit of this version: it lets the
 *                        per-row state of the search live in LDS.
 *   max_distance         only pairs with d <= max_distance (closed); INFINITY = no limit; negative or NaN: GPK_ERR_INVALID_ARGUMENT
 *   flags                GPK_KNN_EXCLUDE_SELF: the pair with r == l + left_row_base is never returned and never counts towards k (a
 *                        column joined against itself, or a row shard of it against the whole).  Unknown bits: GPK_ERR_INVALID_ARGUMENT.
 *                        k, max_distance and flags are checked before any device work.
 *   never matched,       null rows, EMPTY rows (no member has a coordinate) and POINT rows with a NaN coordinate, on either side (the
 *   never candidates     rule of gpk_dwithin_join): such a left row has count 0, such a right row is nobody's neighbour.  An empty right
 *                        side, or one of such rows only, gives no pairs.
 *   out_counts[n_left]   u32 pairs per left row, at most k (may be NULL)
 *   out_pairs[2*cap]     u32 (l, r) interleaved, sorted by (l, d, r): nearest first within a left row (NULL with cap == 0: count-only
 *                        mode)
 *   out_dist[cap]        f64 d(l, r) of each pair (may be NULL)
 *   *n_pairs             total, always set; GPK_ERR_CAPACITY when > cap and pairs were asked for (cap >= n_left * k always suffices).
 *                        More than 2^31 - 1 bbox candidates (right boxes meeting a left box grown by the row's search radius):
 *                        GPK_ERR_CAPACITY, shard the left side.
 * The result does not depend on scheduling: two calls give identical bytes.  `left_row_base` is added to every emitted l.  All buffers
 * live in `out_space`.  `right_index`: an index of `right` carrying the bbox grid (else GPK_ERR_INVALID_ARGUMENT), or NULL: a
 * GPK_INDEX_BBOX_GRID index is built for the call and freed (it is not kept on the handle).  Synchronous, like gpk_spatial_join.
 * Magnitude range: as gpk_distance_rowwise.
 */
#define GPK_KNN_MAX_K 64
#define GPK_KNN_EXCLUDE_SELF 1u
int32_t gpk_knn_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t k, double max_distance,
                     uint32_t flags, uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist,
                     int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream);

/*
 * Within-distance join (GeoPandas sjoin(predicate="dwithin", distance=d)): every (l, r) with distance(left[l], right[r]) <= distance.
 * Left and right are each any of POINT, MULTIPOINT, LINESTRING, MULTILINESTRING, POLYGON, MULTIPOLYGON — all 36 ordered pairs
 * (anything else: GPK_ERR_MISMATCHED_GEOMETRY).
 *   distance             finite and >= 0; negative, NaN or infinite: GPK_ERR_INVALID_ARGUMENT before any device work.  0 is legal and
 *                        means "the closed sets meet" (the exact zero of the distance contract).
 *   the pair test        (l, r) is returned iff d(l, r) <= distance (closed, compared as doubles), where d(l, r) is the library's own
 *                        row-wise distance of the pair: the value the per-row kernel of gpk_distance_rowwise(left, right, ...) computes for
 *                        these two columns — the same device routine, the same lane-group size (chosen from the non-point column when
 *                        one side is POINT, from both columns and the large-row switch otherwise) and the same lane order, so the
 *                        returned distances and the pair set are bit for bit what that call and a comparison would give.  (Its grouped
 *                        schedule for LINESTRING right sides with >= 8 rows per target agrees within its 1e-9 contract.)
 *   never matched        null rows, EMPTY rows (no member has a coordinate) and POINT rows with a NaN coordinate, on either side —
 *                        unlike row-wise distance, which gives 0.0 for a point against an empty linestring
 *   out_counts[n_left]   u32 matches per left row (may be NULL)
 *   out_pairs[2*cap]     u32 (l, r) interleaved, sorted by (l, r) (NULL with cap == 0: count-only mode)
 *   out_dist[cap]        f64 d(l, r) of each pair (may be NULL)
 *   *n_pairs             total, always set; GPK_ERR_CAPACITY when > cap and pairs were asked for.  More than 2^31 - 1 bbox candidates
 *                        (right boxes meeting a left box grown by `distance`) or pairs: GPK_ERR_CAPACITY, shard the left side.
 * `left_row_base` is added to every emitted l.  All buffers live in `out_space`.  `right_index`: an index of `right` carrying the bbox
 * grid (else GPK_ERR_INVALID_ARGUMENT), or NULL: a GPK_INDEX_BBOX_GRID index is built for the call and freed (it is not kept on the
 * handle).  Synchronous, like gpk_spatial_join.  Magnitude range: as gpk_distance_rowwise.
 */
int32_t gpk_dwithin_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double distance,
                         uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist, int64_t pair_capacity,
                         int64_t* n_pairs, int32_t out_space, void* stream);
/* Row-wise dwithin (shapely / GeoPandas GeoSeries.dwithin): out[i] = 1 iff distance(a[i], b[b_rows[i]]) <= distance, else 0; the shape
 * rules of gpk_distance_rowwise (same n without b_rows; b_rows with a POINT column needs the POINT array on the left; an entry out of
 * range behaves like a null row), the `distance` and never-matched rules of gpk_dwithin_join (out[i] = 0).  The distance is the one
 * gpk_distance_rowwise returns for the call, so dwithin(a, b, d)[i] == dwithin(b, a, d)[i] for identity rows.  out[n_geoms(a)] bytes. */
int32_t gpk_dwithin_rowwise(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double distance, uint8_t* out,
                            int32_t out_space, void* stream);

/* ---- line x polygon relations (gpk_linearea.hip) ----------------------------------------------------------------------------------
 * Where a line runs relative to a polygonal geometry.  L = a LINESTRING or MULTILINESTRING row, taken as the closed set of all its
 * segments and coordinates; P = a POLYGON or MULTIPOLYGON row.  The relation is a 3-bit mask: */
#define GPK_LP_INTERIOR 1 /* L has a point in the interior of P (inside a part's shell, outside its holes, off every ring) */
#define GPK_LP_BOUNDARY 2 /* L has a point on a ring of P */
#define GPK_LP_EXTERIOR 4 /* L has a point outside every part of P, or strictly inside a hole */
/* P's interior and exterior are open sets, so every named line / area predicate is a function of the mask alone:
 *   intersects                 mask & 3                      disjoint             mask == 4
 *   covered_by / covers        mask != 0 && !(mask & 4)      within / contains    (mask & 1) && !(mask & 4)
 *   crosses                    (mask & 1) && (mask & 4)      touches              (mask & 2) && !(mask & 1)
 * The mask is EXACT — the set-theoretic answer, decided with exact orientation signs only, no tolerance, the same at any placement of
 * the same figure — for every usable L and every OGC-valid P.  Valid allows rings that touch each other at single points (hole-shell,
 * hole-hole, part-part); a line may pass through such a point, and the side of the piece next to it is judged against the whole
 * geometry.  Rows:
 *   line row unusable      null, no coordinate, or a NaN coordinate: mask 0
 *   degenerate line        a one-coordinate sequence or repeated coordinates: the point set of its coordinates
 *   polygon row unusable   null, or no non-empty member: mask 0
 *   invalid ring           a non-empty ring that is unclosed, has fewer than 4 coordinates, a NaN or no turning extreme vertex: mask 0
 *                          (the rule and the decision of `contains`)
 *   empty members of a multi-geometry are ignored
 *   invalid polygon        (self-crossing rings, overlapping parts) the mask is unspecified; the call terminates normally
 *                          gpk_validity tells which rows are valid, and why the others are not.
 *
 * Row-wise: out_mask[i] = mask(lines[i], polys[poly_rows[i]]).  `lines` is always the first argument.  `poly_rows` (same space as the
 * output) as `b_rows` of gpk_distance_rowwise: NULL = identity (the row counts must then match), an entry >= n_geoms(polys) gives mask
 * 0.  Any other family on either side: GPK_ERR_MISMATCHED_GEOMETRY; a wrong count: GPK_ERR_INVALID_ARGUMENT; both before any device
 * work.  Outputs are stream-ordered (host outputs: the call waits for them).  out_mask[n_geoms(lines)] bytes. */
int32_t gpk_line_polygon_relation(const gpk_geoarray* lines, const gpk_geoarray* polys, const uint32_t* poly_rows, uint8_t* out_mask,
                                  int32_t out_space, void* stream);
#define GPK_LP_PRED_INTERSECTS 0
#define GPK_LP_PRED_WITHIN 1     /* line within polygon == polygon contains line */
#define GPK_LP_PRED_COVERED_BY 2 /* == polygon covers line */
#define GPK_LP_PRED_CROSSES 3
#define GPK_LP_PRED_TOUCHES 4
/* Line x polygon predicate join (GeoPandas sjoin(predicate=...) on roads x districts): every (l, r) whose mask satisfies `predicate`.
 * One side is LINESTRING | MULTILINESTRING and the other POLYGON | MULTIPOLYGON, in either order (any other pair:
 * GPK_ERR_MISMATCHED_GEOMETRY); the predicate names the line / polygon relation whichever side the line is on.  An unknown predicate
 * id: GPK_ERR_INVALID_ARGUMENT.  Unusable rows (mask 0) never match.
 *   out_counts[n_left]   u32 matches per left row (may be NULL)
 *   out_pairs[2*cap]     u32 (l, r) interleaved, sorted by (l, r) (NULL with cap == 0: count-only mode)
 *   out_mask[cap]        u8 the full mask of each pair (may be NULL: a pair's walk then ends as soon as its predicate is settled)
 *   *n_pairs             total, always set; GPK_ERR_CAPACITY when > cap and pairs were asked for
 * `left_row_base` is added to every emitted l.  All buffers live in `out_space`.  `right_index`: an index of `right` carrying the bbox
 * grid (else GPK_ERR_INVALID_ARGUMENT), or NULL: a GPK_INDEX_BBOX_GRID index is built for the call and freed.  Synchronous, like
 * gpk_dwithin_join.  gpk_spatial_join is unchanged: its lines x polygons arm still returns nothing, as the reference's does. */
int32_t gpk_line_polygon_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t predicate,
                              uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, uint8_t* out_mask, int64_t pair_capacity,
                              int64_t* n_pairs, int32_t out_space, void* stream);

/* ---- polygon x polygon relations (gpk_polyrel.hip) --------------------------------------------------------------------------------
 * How two polygonal geometries lie to each other.  A, B = POLYGON or MULTIPOLYGON rows, taken as closed regular sets: the interior
 * (inside a part's shell, outside its holes, off every ring) and the exterior (outside every part, or strictly inside a hole) are
 * open.  The relation is a 4-bit mask: */
#define GPK_PP_INTERIORS 1  /* the interiors of A and B share a point */
#define GPK_PP_BOUNDARIES 2 /* a ring of A and a ring of B share a point */
#define GPK_PP_A_OUTSIDE 4  /* the interior of A has a point in the exterior of B (A is not a subset of B) */
#define GPK_PP_B_OUTSIDE 8  /* the interior of B has a point in the exterior of A (B is not a subset of A) */
/* Every named area / area predicate is a function of the mask alone:
 *   intersects                 mask & 3                       disjoint             mask != 0 && !(mask & 3)
 *   touches                    (mask & 2) && !(mask & 1)      overlaps             (mask & 13) == 13
 *   within / covered_by        (mask & 1) && !(mask & 4)      contains / covers    (mask & 1) && !(mask & 8)
 *   equals                     (mask & 1) && !(mask & 12)     contains_properly    (mask & 11) == 1
 *   crosses                    never
 * A usable pair never has mask 0; only the masks 3, 5, 7, 9, 11, 12, 13, 14 and 15 occur.  mask(B, A) is mask(A, B) with the bits 4
 * and 8 swapped.  The mask is EXACT — the set-theoretic answer, decided with exact orientation signs only, no tolerance, the same at
 * any placement of the same figures — for OGC-valid operands.  Valid allows rings of one geometry that touch each other at single
 * points (hole-shell, hole-hole, part-part), and the other geometry may pass through such a point.  Rows, on either side:
 *   row unusable           null, or no non-empty member: mask 0
 *   invalid ring           a non-empty ring that is unclosed, has fewer than 4 coordinates, a NaN or no turning extreme vertex: mask 0
 *                          (the rule and the decision of `contains`)
 *   empty members of a multi-geometry are ignored
 *   invalid polygon        (self-crossing rings, overlapping parts) the mask is unspecified; the call terminates normally
 *                          gpk_validity tells which rows are valid, and why the others are not.
 *
 * Row-wise: out_mask[i] = mask(a[i], b[b_rows[i]]).  `b_rows` (same space as the output) as in gpk_line_polygon_relation: NULL =
 * identity (the row counts must then match), an entry >= n_geoms(b) gives mask 0.  Any other family on either side:
 * GPK_ERR_MISMATCHED_GEOMETRY; a wrong count: GPK_ERR_INVALID_ARGUMENT; both before any device work.  Outputs are stream-ordered (host
 * outputs: the call waits for them).  out_mask[n_geoms(a)] bytes. */
int32_t gpk_polygon_relation(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, uint8_t* out_mask, int32_t out_space,
                             void* stream);
#define GPK_PP_PRED_INTERSECTS 0
#define GPK_PP_PRED_WITHIN 1 /* left within right (== covered_by: both sets are closed and regular) */
#define GPK_PP_PRED_CONTAINS 2 /* left contains right (== covers) */
#define GPK_PP_PRED_TOUCHES 3
#define GPK_PP_PRED_OVERLAPS 4
#define GPK_PP_PRED_EQUALS 5
#define GPK_PP_PRED_CONTAINS_PROPERLY 6 /* right lies in the interior of left: no shared boundary point */
/* Polygon x polygon predicate join (GeoPandas sjoin(predicate=...) on two polygon tables): every (l, r) whose mask — always A = the
 * left row, B = the right row — satisfies `predicate`.  Both sides POLYGON | MULTIPOLYGON (else GPK_ERR_MISMATCHED_GEOMETRY); an
 * unknown predicate id: GPK_ERR_INVALID_ARGUMENT.  Unusable rows (mask 0) never match.  `left` and `right` may be the same array (a
 * self-join, for adjacency): pair (i, i) then appears for intersects / within / contains / equals and not for touches / overlaps.
 * Outputs (out_counts, out_pairs, out_mask, *n_pairs), the capacity rule, count-only mode, `left_row_base`, `right_index` (NULL: a
 * GPK_INDEX_BBOX_GRID index is built for the call and freed) and the error order are those of gpk_line_polygon_join.  Without out_mask
 * a pair's walk ends as soon as its predicate is settled.  Synchronous.  gpk_spatial_join and gpk_predicate_rowwise are unchanged. */
int32_t gpk_polygon_relation_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t predicate,
                                  uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, uint8_t* out_mask,
                                  int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream);

/* ---- intersection area and length (gpk_overlay.hip) ---------------------------------------------------------------------------------
 * How MUCH two geometries share, without building the intersection geometry (csrc/gpk_overlay.h has the formulation):
 *   a polygonal x b polygonal     out = area(a ∩ b)        (areal interpolation, IoU, overlap share)
 *   a lineal    x b polygonal     out = length(a ∩ b)      (length of road or river inside a zone; b is closed: a piece that runs
 *                                                           along a ring counts; a stretch the line runs over twice counts twice)
 * Every other combination: GPK_ERR_MISMATCHED_GEOMETRY; for polygonal x lineal the message says to swap the arguments.  Each measure
 * is a sum of independent (edge, edge) terms around a pair-local origin.  Shared boundaries (neighbours, a polygon that fills a hole,
 * equal polygons) are decided as for one fixed infinitesimal translation of b by (+eps1, +eps2), eps1 << eps2 — the tie rule: points
 * of a lie below a collinear edge of b and in the x-range (min, max] of an edge of b, points of b above and in [min, max).  Area is
 * continuous under translation, so the limit is the exact area; the length adds back the pieces along ring edges that the translation
 * left outside.  Tolerance, for OGC-valid operands (d = the diagonal of a row's box):
 *   area      |out - exact| <= 1e-9 * (d_a^2 + d_b^2)
 *   length    |out - exact| <= 1e-9 * length(a)
 * at any placement of the figures, georeferenced magnitudes included.  The scale is that of the terms being summed, not of the result,
 * which may be an arbitrarily thin sliver.  Results are >= 0; rows whose boxes are strictly apart give exactly 0.0.  Rows:
 *   row unusable           null, no non-empty member (no coordinate), on either side: NaN
 *   invalid ring           a non-empty ring that fails the ring rule of gpk_polygon_relation: NaN
 *   a line with a NaN or infinite coordinate: NaN
 *   empty members of a multi-geometry are ignored
 *   invalid polygon        (self-crossing rings, overlapping parts) the value is unspecified; the call terminates normally
 *                          gpk_validity tells which rows are valid, and why the others are not.
 *
 * Row-wise: out[i] = measure(a[i], b[b_rows[i]]).  `b_rows` (same space as the output) as in gpk_polygon_relation: NULL = identity
 * (the row counts must then match), an entry >= n_geoms(b) gives NaN.  A wrong count: GPK_ERR_INVALID_ARGUMENT; family and count are
 * checked before any device work.  Outputs are stream-ordered (host outputs: the call waits for them).  out[n_geoms(a)] doubles.  Rows
 * of many thousand coordinates run on the same 16 lanes as any other: correct and slow. */
int32_t gpk_intersection_measure(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double* out, int32_t out_space,
                                 void* stream);
/* Intersection measure join: every (l, r) with measure(left[l], right[r]) > min_measure — strict, on doubles, NaN never hits — and the
 * measure of each pair in out_measure (doubles, pair order; NULL: not wanted).  The families are those of the row-wise call with a =
 * left, b = right.  `min_measure` must be finite and >= 0: anything else is GPK_ERR_INVALID_ARGUMENT before any device work.  At
 * min_measure == 0 a pair that only touches may appear with a value at rounding level: ask for a threshold above the tolerance of
 * the data when touching pairs must stay out.  The measures are bit for bit what the row-wise call gives for the pair.  `left` and
 * `right` may be the same array: pair (i, i) then carries area(i).  Outputs (out_counts, out_pairs, *n_pairs), the capacity rule,
 * count-only mode, `left_row_base`, `right_index` (NULL: a GPK_INDEX_BBOX_GRID index is built for the call and freed) and the error
 * order are those of gpk_polygon_relation_join.  Synchronous. */
int32_t gpk_intersection_measure_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double min_measure,
                                      uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_measure,
                                      int64_t pair_capacity, int64_t* n_pairs, int32_t out_space, void* stream);

/* ---- clip lines to polygons (gpk_lineclip.hip) --------------------------------------------------------------------------------------
 * The piece of a line that lies inside a polygonal geometry, or outside it: GeoPandas GeoSeries.intersection / difference and
 * overlay(how="intersection") on lines x polygons.  csrc/gpk_lineclip.h has the rule. */
#define GPK_CLIP_INSIDE  0   /* L ∩ P, P closed: pieces in P's interior or along a ring */
#define GPK_CLIP_OUTSIDE 1   /* closure of L \ P: pieces in P's exterior (outside every part, or inside a hole) */
#define GPK_CLIP_DROP_EMPTY 1 /* flag */
/* Output row k = clip(lines[line_rows[k]], polys[poly_rows[k]]), k < n_rows.  `lines` LINESTRING | MULTILINESTRING, `polys` POLYGON |
 * MULTIPOLYGON; any other family: GPK_ERR_MISMATCHED_GEOMETRY (for polygonal x lineal the message says to swap the arguments).  A NULL
 * row list is the identity: n_rows must then equal that column's row count.  Both lists live in `rows_space`.  An unknown mode,
 * unknown flag bits, a wrong count, out_src without GPK_CLIP_DROP_EMPTY: GPK_ERR_INVALID_ARGUMENT.  Every refusal comes before any
 * device work.
 *   *out   a callee-owned MULTILINESTRING column that does not view its inputs (free with gpk_geoarray_free): one row per pair, in pair
 *          order.  A part is a maximal run of kept pieces within one coordinate sequence of the line: the run's first point, the
 *          line's coordinates strictly inside it, its last point; parts in the order the line is walked; runs are not merged across
 *          the closing coordinate of a closed sequence nor across members; a stretch the line covers twice is emitted twice.
 *   empty  a pair with no piece of positive length gives a valid row with zero parts
 *   null   (validity 0) for the conditions gpk_intersection_measure answers with NaN — either row null, without a coordinate / a
 *          non-empty member, a ring that fails the ring rule of gpk_polygon_relation, a NaN or infinite line coordinate — and for a row
 *          index past the end of its column
 *   GPK_CLIP_DROP_EMPTY   rows with zero parts and null rows are left out; out_src[k] (int32, `src_space`, may be NULL; room for
 *          n_rows entries) names the input pair of output row k, the part gpk_explode's out_parent plays
 * Every output coordinate is a coordinate of the line or a vertex of the polygon, bit for bit, or a computed crossing within
 * 1e-9 * d of the line's segment and of the ring edge, d = the diagonal of the pair's joint box, at any placement and any crossing
 * angle.  When every two distinct transition points of a segment are at least 1e-6 * |segment| apart, the number of parts and the
 * coordinates per part are those of the exact result; below that the output's point set is within 1e-9 * d of the exact one.  Invalid
 * polygons: unspecified, the call terminates.  A result whose parts or coordinates do not fit i32 offsets: GPK_ERR_INVALID_ARGUMENT (as
 * gpk_geoarray_concat), found after the count pass, nothing stays allocated.  The call waits once, for the sizes of the result; the
 * result's buffers are stream-ordered.  Rows of many thousand coordinates run on the same 16 lanes as any other: correct and slow. */
int32_t gpk_line_clip(const gpk_geoarray* lines, const gpk_geoarray* polys, const uint32_t* line_rows, const uint32_t* poly_rows,
                      int64_t n_rows, int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, void* stream,
                      gpk_geoarray** out);

/* ---- polygon x polygon intersection and difference (gpk_polyclip.hip) ------------------------------------------------------------------
 * The geometry two polygonal rows share, or the part of the first outside the second: GeoPandas overlay(how="intersection") /
 * overlay(how="difference") on polygon layers with keep_geom_type=True.  csrc/gpk_polyclip.h has the rule. */
#define GPK_PCLIP_INTERSECTION 0   /* closure of int(a) ∩ int(b) */
#define GPK_PCLIP_DIFFERENCE   1   /* closure of int(a) \ b      */
/* Output row k = clip(a[a_rows[k]], b[b_rows[k]]), k < n_rows.  Both columns POLYGON | MULTIPOLYGON; any other family:
 * GPK_ERR_MISMATCHED_GEOMETRY.  The row lists, n_rows, rows_space, GPK_CLIP_DROP_EMPTY with out_src, an index past the end of its column
 * (a null row), the refusals — every one before any device work — and their order are those of gpk_line_clip.
 *   *out   a callee-owned MULTIPOLYGON column that does not view its inputs (free with gpk_geoarray_free): one row per pair, in pair
 *          order.  The REGULARISED result, the area part only: points and edges the operands merely share leave no trace.  Rings are
 *          closed, shells counter-clockwise, holes clockwise; a ring starts at its arc with the smallest key (the boundary of a before
 *          that of b, then the order of the walk); parts in the order of their shells' keys, each hole with the shell that encloses it.
 *          Shared boundary comes from a: equal polygons intersect to a, a polygon minus itself is empty, neighbours that share an edge
 *          intersect to nothing.  Parts that touch at a point stay separate rings.
 *   empty  a pair with no area in common (intersection), or with a covered by b (difference), gives a valid row with zero parts
 *   null   (validity 0) for the conditions gpk_intersection_measure answers with NaN, for a row index past the end of its column, and
 *          for a row of status 4
 *   out_status[k] (uint8, `status_space`, may be NULL; always per PAIR, also under GPK_CLIP_DROP_EMPTY):
 *          0 OK; 1 OK, and some output ring touches itself at a point (a hole whose arcs end at a point of its shell fuses into the
 *          shell: the only case in which gpk_validity may object to an output row); 2 empty; 3 null input; 4 unresolved: the arcs did
 *          not close into rings — the row is null, never a guessed geometry.
 * Every output coordinate is a coordinate of a, bit for bit, a coordinate of b, bit for bit, or a computed crossing within 1e-9 * d of
 * both carrying edges, d = the diagonal of the pair's joint box, at any placement and any crossing angle; a crossing has one value
 * wherever it is emitted.  When every two distinct transition points of a segment are at least 1e-6 * |segment| apart, parts, rings,
 * coordinates per ring and ring starts are those of the exact result and status 4 does not occur for OGC-valid operands.  Below that
 * gap either the point set is within 1e-9 * d of the exact one or the row has status 4.  Invalid polygons: unspecified, the call terminates.  The
 * result is identical at every placement, for every lane-group size and on every schedule.  A result whose arcs, parts, rings or
 * coordinates do not fit i32 offsets: GPK_ERR_INVALID_ARGUMENT, found after the counts, nothing stays allocated.  The call waits twice,
 * for the number of arcs and for the sizes of the result; everything else is stream-ordered.  Rows of many thousand coordinates run on
 * the same 16 lanes as any other: correct and slow. */
int32_t gpk_polygon_clip(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows,
                         int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status,
                         int32_t status_space, void* stream, gpk_geoarray** out);

/* ---- polygon x polygon union, and the pairing of a grouped union (gpk_polyunion.hip) -----------------------------------------------------
 * The area either of two polygonal rows covers: GeoPandas GeoSeries.union on polygon columns, area part only.
 * csrc/gpk_polyunion.h has the rule: that of gpk_polygon_clip with another kept table and another choice of a hole's shell. */
#define GPK_PUNION_UNION 0   /* closure of int(a) ∪ int(b), merged across shared boundary */
/* Output row k = union(a[a_rows[k]], b[b_rows[k]]), k < n_rows.  The 14 arguments are those of gpk_polygon_clip, in the same order and
 * with the same meaning, and so is everything but what the mode computes: the families (POLYGON | MULTIPOLYGON on both sides, else
 * GPK_ERR_MISMATCHED_GEOMETRY), the row lists, GPK_CLIP_DROP_EMPTY with out_src, out_status 0 to 4, the refusals — every one before
 * any device work — and their order, the two waits, the i32 offset overflow error, the owned MULTIPOLYGON column, ring orientation,
 * ring starts and part order, and the contract on coordinates (input coordinates bit for bit, crossings within 1e-9 * d of both
 * carrying edges, the gap of 1e-6 * |segment|, below which a row is within 1e-9 * d or null with status 4).  Any other mode:
 * GPK_ERR_INVALID_ARGUMENT.
 *   union  shared boundary comes from a: equal polygons unite to a.  Neighbours that share an edge merge across it; the input
 *          coordinates along a merged edge that end a kept piece stay, collinear or not.  Rows that touch at points only unite to
 *          separate parts, also where they touch twice around a gap (two parts, no hole); a gap closed off by overlap is a hole.  A
 *          hole goes to the INNERMOST shell that encloses it (a shell of a union can lie inside a hole of another one).
 *   null   for the same input conditions as gpk_polygon_clip.  That includes a row without a coordinate on either side: the pair-wise
 *          union does NOT treat an empty row as the neutral element.  Status 2 (empty) does not occur for a row that is not null. */
int32_t gpk_polygon_union(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows,
                          int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status,
                          int32_t status_space, void* stream, gpk_geoarray** out);
/* One round of a grouped union (union_all / dissolve) as a tree reduction over gpk_polygon_union: who is united with whom.  The
 * current rows live in a POOL column (the input rows, then the results of every round, appended with gpk_geoarray_concat), so a row
 * that passes through is not copied.  All buffers on the device, except out_counts.
 *   group[n]  the group id of every current row, ascending;  rows[n]  its pool row (NULL: row i is pool row i)
 *   base      the pool row the result of this round's first pair will have (the pool's length)
 * Within a group, rows 2j and 2j + 1 form pair; an odd last row passes through.  Out, in the order of the current rows:
 *   a_rows, b_rows [n / 2]         the pool rows of every pair: the row lists of this round's gpk_polygon_union over (pool, pool)
 *   next_group, next_rows [n]      the next round's rows: base + k for the result of pair k, its own pool row for a pass-through
 *   out_counts[2] (host)           the number of pairs, the number of rows of the next round: the call's one read-back (it waits once)
 * No pair: the reduction is done.  n < 0 or pool rows past 2^32 - 1: GPK_ERR_INVALID_ARGUMENT. */
int32_t gpk_union_all_pairs(const int32_t* group, const uint32_t* rows, int64_t n, int64_t base, uint32_t* a_rows, uint32_t* b_rows,
                            int32_t* next_group, uint32_t* next_rows, int64_t* out_counts, void* stream);

/* ---- polygon x polygon symmetric difference (gpk_polysymdiff.hip) -----------------------------------------------------------------------
 * The area exactly one of two polygonal rows covers: GeoPandas GeoSeries.symmetric_difference on polygon columns, area part only.
 * csrc/gpk_polysymdiff.h has the rule: that of gpk_polygon_clip with another kept table, a direction per piece, the leftmost turn at
 * proper crossings as well, and the union's choice of a hole's shell. */
#define GPK_PSYMDIFF_SYMMETRIC_DIFFERENCE 0   /* closure of (int(a) \ b) ∪ (int(b) \ a) */
/* Output row k = symmetric_difference(a[a_rows[k]], b[b_rows[k]]), k < n_rows.  The 14 arguments are those of gpk_polygon_clip, in the
 * same order and with the same meaning, and so is everything but what the mode computes: the families (POLYGON | MULTIPOLYGON on both
 * sides, else GPK_ERR_MISMATCHED_GEOMETRY), the row lists, GPK_CLIP_DROP_EMPTY with out_src, out_status 0 to 4, the refusals — every
 * one in the clip's order and before any device work —, the two waits, the i32 offset overflow error, the owned MULTIPOLYGON column,
 * ring orientation, and the contract on coordinates: input coordinates bit for bit, crossings within 1e-9 * d of both carrying edges,
 * the gap of 1e-6 * |segment|, below which a row is within 1e-9 * d or null with status 4.  No covered-by claim is made.  Any other
 * mode: GPK_ERR_INVALID_ARGUMENT.
 *   result equal polygons give an empty row (status 2, zero parts).  Neighbours that share an edge give their union.  b strictly inside
 *          a gives a with b as a hole; a hole goes to the INNERMOST shell that encloses it (a hole of b is a shell inside that hole).
 *          Where the two boundaries cross properly, a \ b and b \ a touch at the crossing and stay separate rings, all of which carry
 *          the one value of that crossing.  A ring starts at its arc with the smallest key, the key of an arc being that of its start
 *          in the direction in which it is emitted (pieces of one boundary inside the other row are emitted backwards).
 *   null   for the same input conditions as gpk_polygon_clip.  That includes a row without a coordinate on either side, as in the
 *          union: an empty row is NOT treated as the neutral element.
 * The result is identical at every placement, for every lane-group size and on every schedule. */
int32_t gpk_polygon_symdiff(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows,
                            int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status,
                            int32_t status_space, void* stream, gpk_geoarray** out);

/* ---- line x line relations (gpk_lineline.hip) ---------------------------------------------------------------------------------------
 * How two lineal geometries lie to each other.  A, B = LINESTRING or MULTILINESTRING rows, each the closed point set of all its
 * segments and coordinates.  Boundary (the mod-2 rule): every non-empty member of a row counts its first and its last coordinate once
 * each; a point counted an odd number of times over the whole row is a boundary point.  A closed member (first = last) counts twice
 * at one point and so contributes none; a member of one coordinate, or of equal coordinates, is a point of the row whose two ends
 * coincide: it has no boundary of its own.  The interior of a row is the row minus its boundary points.  Nothing assumes that a row is
 * simple: the mask is the set-theoretic answer for every usable row, self-crossing ones included.  The relation is a 7-bit mask: */
#define GPK_LL_INTERIORS 1    /* an interior point of A is an interior point of B */
#define GPK_LL_SHARED_PIECE 2 /* A and B share a piece of positive length (always together with GPK_LL_INTERIORS) */
#define GPK_LL_INT_BND 4      /* an interior point of A is a boundary point of B */
#define GPK_LL_BND_INT 8      /* a boundary point of A is an interior point of B */
#define GPK_LL_BND_BND 16     /* a boundary point of A is a boundary point of B */
#define GPK_LL_A_OUTSIDE 32   /* A has a point that is no point of B */
#define GPK_LL_B_OUTSIDE 64   /* B has a point that is no point of A */
/* Every named line / line predicate (DE-9IM, dimension 1 / 1) is a function of the mask alone:
 *   intersects     mask & 31                              disjoint       mask != 0 && !(mask & 31)
 *   touches        (mask & 28) && !(mask & 1)             crosses        (mask & 1) && !(mask & 2)
 *   overlaps       (mask & 2) && (mask & 32) && (mask & 64)
 *   within         (mask & 1) && !(mask & 32)             contains       (mask & 1) && !(mask & 64)
 *   covered_by     (mask & 31) && !(mask & 32)            covers         (mask & 31) && !(mask & 64)
 *   equals         (mask & 1) && !(mask & 96)
 * within and covered_by differ only when A consists of point members that sit on boundary points of B.  A usable pair never has mask
 * 0.  mask(B, A) is mask(A, B) with the bits 4 and 8, and 32 and 64, swapped.  The mask is EXACT: decided with exact orientation signs
 * and coordinate comparisons only, no tolerance, the same at any placement of the same figures.  Rows, on either side:
 *   row unusable           null, no coordinate, or a NaN or infinite coordinate: mask 0, and every predicate is false
 *   empty members are ignored
 *
 * Row-wise: out_mask[i] = mask(a[i], b[b_rows[i]]).  `b_rows` (same space as the output) as in gpk_polygon_relation: NULL = identity
 * (the row counts must then match), an entry >= n_geoms(b) gives mask 0.  Both sides LINESTRING | MULTILINESTRING, any other family
 * on either side: GPK_ERR_MISMATCHED_GEOMETRY; a wrong count: GPK_ERR_INVALID_ARGUMENT; both before any device work.  Outputs are
 * stream-ordered (host outputs: the call waits for them).  out_mask[n_geoms(a)] bytes.  Rows of many thousand coordinates run on the
 * same 16 lanes as any other: correct and slow. */
int32_t gpk_line_relation(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, uint8_t* out_mask, int32_t out_space,
                          void* stream);
#define GPK_LL_PRED_INTERSECTS 0
#define GPK_LL_PRED_WITHIN 1
#define GPK_LL_PRED_CONTAINS 2
#define GPK_LL_PRED_COVERED_BY 3
#define GPK_LL_PRED_COVERS 4
#define GPK_LL_PRED_CROSSES 5
#define GPK_LL_PRED_TOUCHES 6
#define GPK_LL_PRED_OVERLAPS 7
#define GPK_LL_PRED_EQUALS 8
/* Line x line predicate join (GeoPandas sjoin(predicate=...) on two line tables): every (l, r) whose mask — always A = the left row,
 * B = the right row — satisfies `predicate`.  Both sides LINESTRING | MULTILINESTRING (else GPK_ERR_MISMATCHED_GEOMETRY); an unknown
 * predicate id: GPK_ERR_INVALID_ARGUMENT.  Unusable rows (mask 0) never match.  `left` and `right` may be the same array (a self-join,
 * for junctions and duplicates): pair (i, i) then appears for intersects / equals / within / contains / covered_by / covers and not
 * for touches / crosses / overlaps.  Outputs (out_counts, out_pairs, out_mask, *n_pairs), the capacity rule, count-only mode,
 * `left_row_base`, `right_index` (NULL: a GPK_INDEX_BBOX_GRID index is built for the call and freed) and the error order are those of
 * gpk_polygon_relation_join.  Without out_mask a pair's work ends as soon as its predicate is settled.  Synchronous.
 * gpk_spatial_join, gpk_line_polygon_relation / _join and gpk_predicate_rowwise are unchanged. */
int32_t gpk_line_relation_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t predicate,
                               uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, uint8_t* out_mask, int64_t pair_capacity,
                               int64_t* n_pairs, int32_t out_space, void* stream);

/* ---- point relations (gpk_pointrel.hip) -----------------------------------------------------------------------------------------------
 * How a punctual geometry lies to a geometry of any family.  A = a POINT or MULTIPOINT row, the finite set of its points; B = a row of
 * any of the six families.  The relation is a 4-bit mask: */
#define GPK_PT_INTERIOR 1  /* a point of A lies in the interior of B */
#define GPK_PT_BOUNDARY 2  /* a point of A lies on the boundary of B */
#define GPK_PT_EXTERIOR 4  /* a point of A is no point of B */
#define GPK_PT_B_OUTSIDE 8 /* B has a point that is no point of A */
/* Interior and boundary of B are those of the sibling relations:
 *   punctual B     every point is interior, there is no boundary; bit 8: some point of B equals no point of A (exact coordinate
 *                  comparison; duplicates and member order do not matter)
 *   lineal B       the closed point set of its segments and coordinates with the mod-2 boundary of gpk_line_relation; a member of one
 *                  coordinate or of equal coordinates is a point of the row without a boundary.  Bit 8 unless every member of B is
 *                  such a point and each of them is a point of A.  Nothing assumes B is simple.
 *   polygonal B    the point sets of gpk_polygon_relation: interior = inside a part's shell, outside its holes and off every ring;
 *                  boundary = on a ring; exterior = outside every part or strictly inside a hole.  Exact for OGC-valid rows (rings
 *                  that touch at points are allowed, and a point of A may sit on such a point: boundary); bit 8 is always set.  For an
 *                  invalid polygon the mask is unspecified and the call terminates
 *                  (gpk_validity says which rows are valid).
 * This is DE-9IM with dim(A) = 0 and an empty boundary of A: II, IB, IE are the bits 1, 2, 4, and bit 8 is "EI or EB non-empty".
 * Every named predicate is a function of the mask and of the dimension of B's FAMILY (0, 1, 2 by column type, not by degeneracy):
 *   intersects     mask & 3                               disjoint       mask != 0 && !(mask & 3)
 *   within         (mask & 1) && !(mask & 4)              covered_by     (mask & 3) && !(mask & 4)
 *   contains       (mask & 1) && !(mask & 8)              covers         (mask & 3) && !(mask & 8)      (A contains / covers B)
 *   touches        (mask & 2) && !(mask & 1)              equals         (mask & 1) && !(mask & 12)
 *   crosses        dim(B) >= 1: (mask & 1) && (mask & 4);  dim(B) == 0: never
 *   overlaps       dim(B) == 0: (mask & 13) == 13;         dim(B) >= 1: never
 * For two punctual rows mask(B, A) is mask(A, B) with the bits 4 and 8 swapped.  A usable pair never has mask 0; the masks that occur
 * are 1, 5, 9, 12, 13 for a punctual B, 9 .. 15 for a polygonal B, 9 .. 15 and (all members degenerate) 1, 5 for a lineal B.  The mask
 * is EXACT: exact orientation signs and coordinate comparisons only, no tolerance, the same at any placement.  Rows, on either side:
 *   row unusable           null, no coordinate, a NaN or infinite coordinate (a POINT with NaN is the empty point), a polygon ring that
 *                          fails the ring rule of `contains`: mask 0, and every predicate is false
 *   empty members are ignored
 *
 * Row-wise: out_mask[i] = mask(points[i], other[other_rows[i]]).  `points` POINT | MULTIPOINT, `other` any of the six families, anything
 * else GPK_ERR_MISMATCHED_GEOMETRY; `other_rows` (same space as the output) as b_rows of gpk_line_relation: NULL = identity (the row
 * counts must then match, else GPK_ERR_INVALID_ARGUMENT), an entry >= n_geoms(other) gives mask 0; all before any device work.
 * Outputs are stream-ordered (host outputs: the call waits for them).  out_mask[n_geoms(points)] bytes. */
int32_t gpk_point_relation(const gpk_geoarray* points, const gpk_geoarray* other, const uint32_t* other_rows, uint8_t* out_mask,
                           int32_t out_space, void* stream);
#define GPK_PT_PRED_INTERSECTS 0
#define GPK_PT_PRED_WITHIN 1
#define GPK_PT_PRED_CONTAINS 2
#define GPK_PT_PRED_COVERED_BY 3
#define GPK_PT_PRED_COVERS 4
#define GPK_PT_PRED_CROSSES 5
#define GPK_PT_PRED_TOUCHES 6
#define GPK_PT_PRED_OVERLAPS 7
#define GPK_PT_PRED_EQUALS 8
/* Point predicate join (GeoPandas sjoin(points, ..., predicate=...)): every (l, r) with "left row PREDICATE right row".  At least one
 * side must be POINT | MULTIPOINT, else GPK_ERR_MISMATCHED_GEOMETRY (the message names the join of the two families); an unknown
 * predicate id: GPK_ERR_INVALID_ARGUMENT, checked first.  A is the punctual side — the left one when both are — and out_mask is always
 * the mask with that A; when only the right side is punctual the transposed predicate is evaluated (within <-> contains, covered_by
 * <-> covers, the rest read the same both ways).  A predicate that can never hold for the pair of families (overlaps against a line or
 * a polygon, crosses between points) is a valid call with zero pairs.  Unusable rows never match.  `left` and `right` may be the same
 * array (duplicates of a point table): pair (i, i) then appears for intersects / equals / within / contains / covered_by / covers.
 * Outputs (out_counts, out_pairs, out_mask, *n_pairs), the capacity rule, count-only mode, `left_row_base`, `right_index` (NULL: a
 * GPK_INDEX_BBOX_GRID index is built for the call and freed) and the error order are those of gpk_line_relation_join.  Without
 * out_mask a pair's work ends as soon as its predicate is settled.  Synchronous.  gpk_spatial_join, gpk_predicate_rowwise and every
 * other call are unchanged. */
int32_t gpk_point_relation_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t predicate,
                                uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, uint8_t* out_mask, int64_t pair_capacity,
                                int64_t* n_pairs, int32_t out_space, void* stream);

/* ---- validity and simplicity (gpk_validity.hip) -------------------------------------------------------------------------------------
 * Is a polygonal row OGC-valid — the condition under which the relation masks above are exact — and if not, why not and where.
 * `a` is a POLYGON or MULTIPOLYGON column (any other family: GPK_ERR_MISMATCHED_GEOMETRY, before any device work).  Only the non-empty
 * members of a row (at least one ring, a non-empty shell) and their non-empty rings count, as in the relation calls.  The code of a
 * row is the LOWEST one that applies, so each code is stated for rows to which no lower one applies: */
#define GPK_VALID 0                          /* none of the codes below; a row without a non-empty member is valid */
#define GPK_INVALID_COORDINATE 1             /* a coordinate is NaN or infinite */
#define GPK_INVALID_RING_SHAPE 2             /* a ring has fewer than 4 coordinates, or its first and last coordinates differ */
#define GPK_INVALID_RING_SELF_INTERSECTION 3 /* within one ring, zero-length segments dropped: two consecutive segments share more than
                                              * their common end point, or two others share any point (the closing vertex joins the last
                                              * and the first segment); also spikes, all-collinear rings, a ring of equal coordinates */
#define GPK_INVALID_RINGS_CROSS 4            /* two rings of the row share a piece of positive length, or one has points strictly inside
                                              * and strictly outside the other */
#define GPK_INVALID_HOLE_OUTSIDE_SHELL 5     /* a hole has a point strictly outside its member's shell */
#define GPK_INVALID_NESTED_HOLES 6           /* a hole has a point strictly inside another hole of its member */
#define GPK_INVALID_NESTED_MEMBERS 7         /* the interiors of two members share a point (a shell inside a hole of another member,
                                              * touching it at single points at most, is valid) */
#define GPK_INVALID_DISCONNECTED_INTERIOR 8  /* the interior of a member is not connected: the graph of its rings and of the distinct
                                              * points where two or more of them touch has a cycle */
#define GPK_INVALID_NULL 9                   /* the row is null */
/* Every ring that the relation calls reject (their "invalid ring" rule) has a code from 1 to 3.  out_where[i] (may be NULL) is an index
 * into the column's coordinate buffer, -1 for the codes 0 and 9:
 *   1      the lowest offending coordinate             2      the first coordinate of the lowest offending ring
 *   3, 4   the lowest i such that the segment starting at coordinate i takes part in such a fault: it shares the forbidden point or
 *          piece with another segment of its ring (3), it shares a piece with a segment of another ring, or it passes through a point
 *          where its ring changes sides of another ring or leaves it after running along it (4); for a ring of equal coordinates
 *          only (3) its first coordinate
 *   5, 6   the first coordinate of the lowest-numbered offending hole (6: the hole that lies inside another one)
 *   7      the first coordinate of the lowest-numbered member whose interior meets the interior of a lower-numbered member
 *   8      the first coordinate of the lowest-numbered member whose interior is not connected
 * Every decision is an exact orientation sign or an exact coordinate comparison: no tolerance, the same answer at any placement of the
 * same figure.  Stream-ordered (a host output: the call waits for it); nothing is done for a column without rows.
 * out_code[n_geoms(a)] bytes, out_where[n_geoms(a)] int32. */
int32_t gpk_validity(const gpk_geoarray* a, uint8_t* out_code, int32_t* out_where, int32_t out_space, void* stream);
/* Is a lineal row simple.  `a` is a LINESTRING or MULTILINESTRING column (any other family: GPK_ERR_MISMATCHED_GEOMETRY).  out[i] = 1
 * when, with zero-length segments dropped, (a) in every member consecutive segments share only their common end point and other
 * segments share nothing, except that the first and the last segment of a closed member share its start, and (b) two members share
 * only points that are end points of both — a closed member has no end points.  A member of one coordinate or of equal coordinates is
 * a point: it has no segments and takes part in neither rule.  A row without coordinates is simple.  out[i] = 0 otherwise, and for a
 * null row and a row with a NaN or infinite coordinate.  Exact, stream-ordered and sized like gpk_validity.  out[n_geoms(a)] bytes. */
int32_t gpk_is_simple(const gpk_geoarray* a, uint8_t* out, int32_t out_space, void* stream);

/* ---- triangulation (gpk_triangulate.hip, the rule: csrc/gpk_triangulate.h) -----------------------------------------------------------
 * Every polygonal row as triangles over the column's own coordinates: an index buffer for a renderer or a mesh consumer.  `a` is a
 * POLYGON or MULTIPOLYGON column (any other family: GPK_ERR_MISMATCHED_GEOMETRY, before any device work); both coordinate layouts of an
 * upload are accepted.  Exact ear clipping: holes are bridged into their shell, rings that touch are split at the touch first.  Every
 * decision is an exact orientation sign or a coordinate comparison and every choice goes to the lowest node: no tolerance.
 *   out_tri_offsets[n_geoms + 1]  int32, row i owns triangles out_tri_offsets[i] .. out_tri_offsets[i + 1]
 *   out_index[3 * tri_capacity]   u32 indices into the column's coordinate buffer — the index space of gpk_validity's out_where —
 *                                 three a triangle.  NULL: the size query; offsets, status and *n_triangles are still produced.
 *   out_status[n_geoms]           u8 GPK_TRI_* (may be NULL)
 *   *n_triangles                  the total, always set; GPK_ERR_CAPACITY when > tri_capacity and indices were asked for.
 *                                 tri_capacity >= n_coords(a) + 3 * n_rings(a) always suffices: the same expression over one row is
 *                                 that row's SHARE, a row that would need more is GPK_TRI_FAILED and never writes past it.
 * Guarantee, for every row gpk_validity gives code 0, at any placement and for either winding of the input rings:
 *   (a) every index is a coordinate of that row and never a ring's closing coordinate (the ring's first coordinate stands for it);
 *   (b) every triangle has strictly positive exact orientation;
 *   (c) the triangulation is conforming on the row's vertex set: by coordinate value a directed triangle edge occurs at most once, an
 *       edge whose reverse does not occur lies on a ring edge, and no vertex of the row lies in the open interior of a triangle edge
 *       — no T-junctions, also where a hole touches a shell edge mid-segment or two members touch;
 *   (d) the exact sum of the triangle areas is the exact area of the row; every member is triangulated on its own;
 *   (e) a member none of whose rings share a point gives N' + 2 h - 2 triangles (N': its ring positions without closing coordinates and
 *       consecutive repeats, h: its holes); with s (vertex, open edge of another ring) incidences at most N' + s + 2 h - 2;
 *   (f) the indices are a function of the figure: identical across lane-group sizes and the work-group path, coordinate layouts, host
 *       and device buffers, repeated calls, exact translations and power-of-two scalings.
 * Limits: a valid row whose MEMBERS touch each other in so many points that its nodes pass the share (more than 3 per ring of the
 * row) is GPK_TRI_FAILED.  A row whose share exceeds 5000 (TRI_LDS_NODES) keeps its list in global scratch, not in LDS: correct and
 * slow, and the call then takes 32 bytes of scratch per unit of the column's share on top of the 12 it always takes.  Invalid rows (any other validity code — GeoSeries.is_valid tells): the answer is unspecified, the call
 * terminates, indices stay inside the row, the count inside the share; a row that stalls is GPK_TRI_FAILED with zero triangles.
 * Stream-ordered, with one read-back (the total).  All outputs live in `out_space`. */
#define GPK_TRI_OK     0 /* the row's triangles are written */
#define GPK_TRI_EMPTY  1 /* null row, or no non-empty member: zero triangles */
#define GPK_TRI_FAILED 2 /* zero triangles: a NaN / infinite coordinate, a ring that fails the ring rule of gpk_polygon_relation,
                            a row that needs more than its share, or clipping / bridging could not finish (only invalid rows) */
int32_t gpk_triangulate(const gpk_geoarray* a, uint32_t* out_index, int64_t tri_capacity, int32_t* out_tri_offsets, uint8_t* out_status,
                        int64_t* n_triangles, int32_t out_space, void* stream);

/* ---- linear referencing (gpk_linref.hip) ------------------------------------------------------------------------------------
 * Where on a geometry the nearest point lies, how far along a line it is, and the point at a measure along a line (geo 0.27
 * ClosestPoint / LineLocatePoint / LineInterpolatePoint; shapely / GeoPandas nearest_points, shortest_line, project, interpolate).
 * Shape rules of all three: the POINT column is the first argument; `b_rows` / `line_rows` (same space as the outputs) as in
 * gpk_distance_rowwise — NULL = identity (the row counts must then match), an entry >= n_geoms behaves like a null row; any other
 * geometry family than the ones named gives GPK_ERR_MISMATCHED_GEOMETRY, a wrong count GPK_ERR_INVALID_ARGUMENT, both before any
 * device work.  Outputs are stream-ordered (host outputs: the call waits for them).  Magnitude range: as gpk_distance_rowwise.
 *
 * Closest point: q[i] = the point of B = b[b_rows[i]] nearest to p = a[i]; a POINT, b any of the six families.
 *   - B polygonal and p inside or on its boundary (the exact position test of `distance`, holes excluded): q = p bit for bit, seg = -1;
 *   - otherwise the candidates are every segment of every coordinate sequence of B (all rings of all parts, all member linestrings;
 *     a MULTIPOINT member, a POINT and a one-coordinate sequence are degenerate segments), compared as gpk_distance_rowwise compares
 *     them (squared distances as fractions).  Ties: the winner is the minimising segment with the LOWEST start index in b's
 *     coordinate buffer, whatever the lane-group size; out_seg[i] (may be NULL) is that coordinate index;
 *   - with s, e the winner's ends, dot = (p - s).(e - s), d2 = |e - s|^2: q = s when dot <= 0 or d2 == 0, q = e when dot >= d2 (both
 *     bit for bit), else s + (dot / d2)(e - s): each component within 2^-48 max(|p|, |s|, |e|) (largest coordinate magnitudes) of the
 *     exact nearest point of that segment;
 *   - a null or empty row on either side or a NaN point: q = (NaN, NaN), seg = -1.  out_xy[2 n] interleaved, n = n_geoms(a). */
int32_t gpk_closest_point_rowwise(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double* out_xy, int32_t* out_seg,
                                  int32_t out_space, void* stream);
/* Locate (project): out[i] = the measure along lines[line_rows[i]] of its point nearest to pts[i]; pts POINT, lines LINESTRING |
 * MULTILINESTRING.  The winning segment is the closest-point winner (same scan, same tie rule); the measure is the summed length of
 * every segment before it in storage order plus the length from its start to q.  MULTILINESTRING: members are measured consecutively
 * in storage order (GEOS LengthIndexedLine), empty members are skipped, the gap between two members has no length.  normalized != 0
 * divides by the total length (a line without length: 0.0).  Null or empty rows and NaN points give NaN.  Within 1e-9 x the line's
 * length of the exact measure of the winning segment's nearest point.  out[n_geoms(pts)]. */
int32_t gpk_line_locate_point(const gpk_geoarray* pts, const gpk_geoarray* lines, const uint32_t* line_rows, int32_t normalized, double* out,
                              int32_t out_space, void* stream);
/* Interpolate: the point at measure distances[i] along lines[i] (LINESTRING | MULTILINESTRING, measured as by locate).  `distances`
 * lives in out_space; n_distances is 1 (one value for every row: it is not expanded to n values) or n_geoms(lines).  With L the
 * line's length: a normalized distance is multiplied by L first, d < 0 is measured from the end (d += L), the result is clamped to
 * [0, L].  The point lies on the first segment in storage order whose cumulative end measure is >= d; a measure that lands exactly on
 * a vertex returns that vertex bit for bit (at a member boundary: the end of the earlier member); L == 0 gives the first coordinate.
 * A NaN distance and a null or empty line give (NaN, NaN) and out_valid 0.  Within 1e-9 L of the exact point, per component.
 * out_xy[2 n] interleaved, out_valid[n] bytes 0/1 (may be NULL). */
int32_t gpk_line_interpolate_point(const gpk_geoarray* lines, const double* distances, int64_t n_distances, int32_t normalized,
                                   double* out_xy, uint8_t* out_valid, int32_t out_space, void* stream);

/*
 * Stream-ordered form of gpk_spatial_join for callers that keep everything in HBM (the idiom a pipeline of
 * kernels on one HIP stream wants; the reference's call is synchronous, spatial_index.rs:44-58): the join is
 * ENQUEUED on `stream` and the call returns without waiting.
 *   - point x polygon / multipolygon only, `right_index` required (nothing to build or free behind the stream);
 *   - out_counts / out_pairs are device buffers (either may be NULL as above);
 *   - *n_pairs_dev (device or device-mapped host memory, may be NULL) receives the total number of hits when the
 *     stream reaches that point; pairs beyond pair_capacity are dropped, so compare the two after synchronising.
 * Scratch comes from an arena owned by (calling thread, stream): calls enqueued on different streams do not share
 * buffers; calls on ONE stream reuse them in stream order.
 */
int32_t gpk_spatial_join_async(const gpk_geoarray* left, const gpk_geoarray* right,
                               const gpk_index* right_index, int32_t predicate, uint32_t left_row_base,
                               uint32_t* out_counts, uint32_t* out_pairs, int64_t pair_capacity,
                               int64_t* n_pairs_dev, void* stream);

/* ---- join assembly (spatial_index.rs:145-203) ------------------------------------------------ */
/* The reference turns the (l, r) pairs into two u64 index Series and lets polars `inner_join` / `left_join` pull
 * the attribute columns (spatial_index.rs:147-199).  Here: the row indices of the joined table, then a gather per
 * column.  All buffers of one call live in `space`. */
#define GPK_JOIN_INNER 0
#define GPK_JOIN_LEFT  1
/* (counts[n_left], sorted pairs[2*n_pairs] as produced by gpk_spatial_join with `left_row_base`) -> out_l / out_r
 * [capacity] i64 row indices, sorted by l.  Left join: a left row without hits appears once with r = -1
 * (JoinType::Left, spatial_index.rs:186-199); other join types do not exist upstream (:200-202).
 * *n_rows is always set (capacity 0 = size query; GPK_ERR_CAPACITY when it does not fit). */
int32_t gpk_join_indices(const uint32_t* counts, const uint32_t* pairs, int64_t n_left, int64_t n_pairs,
                         uint32_t left_row_base, int32_t join_type, int64_t* out_l, int64_t* out_r,
                         int64_t capacity, int64_t* n_rows, int32_t space, void* stream);
/* out[i] = values[idx[i]] for a fixed-width Arrow column (elem_bits 1 = boolean bitmap, 8, 16, 32, 64, 128);
 * idx[i] = -1 (or out of range) and null source rows give a null: out_validity (Arrow bitmap, may be NULL). */
int32_t gpk_take_fixed(const void* values, int32_t elem_bits, const uint8_t* validity, int64_t n_values,
                       const int64_t* idx, int64_t n_idx, void* out_values, uint8_t* out_validity,
                       int32_t space, void* stream);
/* The same for an Arrow Binary / Utf8 column (i32 offsets + bytes; the reference's geometry column is one).
 * out_offsets[n_idx + 1]; out_values NULL + capacity 0 = size query; *n_bytes always set. */
int32_t gpk_take_binary(const uint8_t* values, const int32_t* offsets, const uint8_t* validity, int64_t n_values,
                        const int64_t* idx, int64_t n_idx, int32_t* out_offsets, uint8_t* out_values,
                        int64_t capacity, int64_t* n_bytes, uint8_t* out_validity, int32_t space, void* stream);

/* ---- rows of a geometry column (gpk_geotake.hip, the rule: csrc/gpk_geotake.h) ---------------------------------------------------------
 * take: output row i is source row idx[i] — any order, repeats allowed — for every one of the six geometry types; the result has the
 * source's type and is a new handle that owns all of its buffers (gpk_geoarray_free; the source may be freed first).  What a dataframe
 * does to every column (take, filter, slice, head), and the gather of a join's geometry columns without a detour through WKB.
 *   - Everything is copied bit for bit: coordinates with their NaN payloads and signed zeros, and the children of a null source row
 *     too.  All offsets start at 0.
 *   - An index of -1, or any index outside [0, n), gives a null row without children (the convention of gpk_take_fixed; a left join's
 *     r = -1); in a POINT column that row's coordinate is (NaN, NaN).
 *   - The result has a validity bitmap if the source has one or some index is out of range; otherwise it has none.
 *   - idx lives in idx_space (GPK_MEM_HOST or GPK_MEM_DEVICE).  n_idx == 0 gives a column of zero rows.
 *   - The call waits once, for one small read-back (the child totals of every level and the count of out-of-range indices); everything
 *     else is stream-ordered.
 *   - A level whose total exceeds 2^31 - 1 is refused (GPK_ERR_INVALID_ARGUMENT, Arrow i32 offsets) before anything is allocated.
 *   - Refused before any device work, with *out = NULL: a NULL a or out, a NULL idx with n_idx > 0, a negative n_idx, an unknown space.
 * Schedule: count -> scan -> one wait -> fill; the fill works in output order, one work-group per strip of 1024 output elements, so a
 * row of one coordinate and a row of 10^5 move at the same rate. */
int32_t gpk_geoarray_take(const gpk_geoarray* a, const int64_t* idx, int64_t n_idx, int32_t idx_space, void* stream, gpk_geoarray** out);
/* filter: the rows the mask keeps, in source order, under exactly the contract of take.  mask has one entry per source row, in
 * mask_space: mask_bits == 1 is an Arrow bitmap (LSB first), mask_bits == 8 a byte per row (nonzero keeps the row); any other value
 * is refused.  *n_kept is always set.  The kept row numbers are compacted on the device and never visit the host; the compaction is
 * part of the counting pass, so filter also waits once.  The mask has no validity of its own: a caller with a nullable mask ANDs the
 * two bitmaps first. */
int32_t gpk_geoarray_filter(const gpk_geoarray* a, const uint8_t* mask, int32_t mask_bits, int32_t mask_space, void* stream, gpk_geoarray** out, int64_t* n_kept);

/* ---- edits of coordinate sequences (gpk_seqedit.hip, the rule: csrc/gpk_seqedit.h) ------------------------------------------------------
 * Four operations that rewrite the vertices of a column on the device.  Common to all four:
 *   - Every geometry type is accepted.  *out is a callee-owned column of the same type and the same number of rows; it does not view a
 *     and is freed with gpk_geoarray_free; a may be freed first.
 *   - Every offsets level above the innermost one is copied unchanged; only the innermost offsets and the coordinates are rewritten.
 *   - Null rows stay null (their children are edited like any others), and the result has a validity bitmap exactly when a has one.
 *   - Empty rows, parts without rings and sequences without coordinates keep their (empty) slots.
 *   - A SEQUENCE is a LINESTRING row, a member of a MULTILINESTRING, a ring of a POLYGON or MULTIPOLYGON, or a single coordinate of a
 *     POINT or MULTIPOINT column: point columns pass through every operation as a bit-for-bit copy.
 *   - Coordinates that are not computed are moved as 16 bytes: NaN payloads and signed zeros survive.
 *   - Refusals come before any device work and leave *out untouched: a NULL a, a NULL out, and the argument rules below.
 *   - A result whose coordinates do not fit i32 offsets returns GPK_ERR_INVALID_ARGUMENT: found after the count, before anything is
 *     allocated, *out untouched.
 *   - segmentize and remove_repeated_points wait once, for the coordinate total; reverse and orient_polygons do not wait at all.
 *     Everything else is stream-ordered. */
/* segmentize (GeoSeries.segmentize, geo's Densify): a segment p -> q of a sequence is split into n equal pieces.  With dx = qx - px,
 * dy = qy - py, len = sqrt(dx*dx + dy*dy): n = 1 if !(len > m) or len is not finite, otherwise n = min(ceil(len / m), 2^31).  The new
 * coordinates are (px + dx * t, py + dy * t), t = (double)j / (double)n, for j = 1 .. n - 1: exactly these operations in this order,
 * no contraction; the division is j / n, not j * (1 / n) and not a walked sum — the library's own definition (geo and GEOS differ from
 * it, and from each other, in the last bit).  p and q themselves are copied bit for bit, so closed rings stay closed.
 * m is max_segment_length when per_row == NULL, else per_row[row]: one f64 per row of a, in per_row_space (GPK_MEM_HOST or
 * GPK_MEM_DEVICE; max_segment_length is then ignored).  A scalar m that is NaN or <= 0 is refused; a per-row value that is NaN or <= 0
 * leaves that row unchanged (the array is not read back to check it).  The piece counts are summed in 64 bits: one segment with
 * len / m = 1e10 is a clean GPK_ERR_INVALID_ARGUMENT, not a wrap. */
int32_t gpk_segmentize(const gpk_geoarray* a, double max_segment_length, const double* per_row, int32_t per_row_space, void* stream, gpk_geoarray** out);
/* remove_repeated_points (geo's RemoveRepeatedPoints): coordinate c of a sequence is kept iff it is the sequence's first or
 * !(x[c] == x[c-1] && y[c] == y[c-1]).  The comparison is numeric: -0.0 == 0.0, and a NaN coordinate is never a repeat.  Repeats
 * across a sequence boundary are not removed.  A ring that collapses keeps what is left: [A, A, A, A] -> [A].  tolerance must be
 * exactly 0.0: any other value, NaN included, is refused (a positive tolerance is sequential along the sequence and its end rule
 * differs between GEOS versions; the argument exists so that the signature need not change). */
int32_t gpk_remove_repeated_points(const gpk_geoarray* a, double tolerance, void* stream, gpk_geoarray** out);
/* reverse: every sequence's coordinates in reverse order, out[lo + k] = in[hi - 1 - k]; the order of sequences, parts and rows is
 * unchanged, and so are POINT and MULTIPOINT columns. */
int32_t gpk_reverse(const gpk_geoarray* a, void* stream, gpk_geoarray** out);
/* orient_polygons (geo's Orient): POLYGON and MULTIPOLYGON columns; the first ring of every polygon is the shell, the others are holes.
 * The turn of a ring is taken at its lexicographically smallest coordinate v — smallest x, then smallest y, the lowest index among
 * equals; the closing coordinate is not a candidate — between u, the nearest coordinate before v (cyclically) that differs from v, and
 * w, the nearest after v that differs from v: s is the EXACT sign of orient(u, v, w) (filter + expansion, not the f64 shoelace sum),
 * s > 0 counter-clockwise.  A ring is reversed, as by gpk_reverse, iff s != 0 and its direction is not the one wanted: shells CCW and
 * holes CW by default, the opposite with exterior_cw = 1; any other value is refused.  Copied unchanged: rings with s == 0 (a spike at
 * v, or fewer than three distinct coordinates), rings with a non-finite coordinate, rings of fewer than 4 coordinates.  For every ring
 * gpk_validity accepts, s is the ring's orientation (v is a convex corner of a simple ring).  The result is identical at any placement
 * and on every schedule.  Every other geometry type gets a bit-for-bit copy. */
int32_t gpk_orient_polygons(const gpk_geoarray* a, int32_t exterior_cw, void* stream, gpk_geoarray** out);

/* ---- chunked columns ------------------------------------------------------------------------------------ */
/* K chunks of one column held by this process -> ONE array (a new handle, gpk_geoarray_free): Arrow's rechunk — the reference turns
 * every Series into a single chunk before it looks at it (py-geopolars/src/ffi.rs:56,73,93).  Device-resident: the chunks' buffers
 * are placed with device copies, offsets rebased (a chunk's offsets need not start at 0: a sliced Arrow array), validity bits
 * repacked across chunk boundaries that do not fall on a byte.  The placement / rebase / repack code is the all-gatherv's own
 * (below): what runs here with K chunks is what runs there with K ranks.  All chunks must have the same geometry type
 * (GPK_ERR_MISMATCHED_GEOMETRY); 1 <= n_chunks <= 64.  out_row_bases[n_chunks + 1] (host, may be NULL): first row of every chunk. */
int32_t gpk_geoarray_concat(const gpk_geoarray* const* chunks, int32_t n_chunks, void* stream, gpk_geoarray** out,
                            int64_t* out_row_bases, int64_t* out_bytes);

/* ---- multi-GPU: the one collective of the path ------------------------------------ */
/* One process per GPU; the LEFT series is sharded by rows and needs no collective (disjoint output rows, pairs carry
 * `left_row_base`).  A RIGHT side that is itself produced sharded is exchanged once — where `spatial_join` receives its right
 * side and its index, spatial_index.rs:37-76 — with an all-gatherv of its GeoArrow buffers over RCCL / xGMI, and the leaves of
 * its index (per-geometry boxes: the NodeEnvelopes of spatial_index.rs:206-312, gpk_bounds of the shard) travel the same way,
 * so that gpk_index_build_ex assembles the gathered index from them.  Device-resident end to end: lengths first (one small
 * all-gather, the only host read), then one grouped round of broadcasts per buffer with every piece landing at its final
 * offset; offsets are rebased and validity repacked on the device.  RCCL is opened at run time (GPK_RCCL_PATH, else the
 * copy the process already holds, else the system's): there is no link-time dependency.
 *   gpk_comm_unique_id   rank 0 draws the 128-byte id (ncclUniqueId) and hands it to the other ranks by any side channel
 *   gpk_comm_init        every rank, same id: a communicator on the current device (collective call)
 *   gpk_allgatherv_geoarray   shard -> the whole column in rank order (a new handle, gpk_geoarray_free); *out_row_base = first
 *                        row of this rank's shard in it; every rank passes the same geometry type (GPK_ERR_MISMATCHED_GEOMETRY)
 *   gpk_allgatherv_rows_f64   n_local rows of `width` doubles (device) -> all rows in rank order; out_dev NULL = total only
 *                        (still a collective: every rank must make the same call); out_counts[world] host, may be NULL */
typedef struct gpk_comm gpk_comm;
int32_t gpk_comm_unique_id(uint8_t out_id[128]);
int32_t gpk_comm_init(int32_t rank, int32_t world, const uint8_t id[128], gpk_comm** out);
int32_t gpk_comm_free(gpk_comm* comm);
int32_t gpk_comm_info(const gpk_comm* comm, int32_t* out_rank, int32_t* out_world);
/* An IN-PROCESS transport for tests of the exchange (no RCCL): `world` threads of one process on one device stand in for the ranks.
 * gpk_comm_mock_world makes the meeting place, every thread opens its communicator on it with gpk_comm_init_mock and calls
 * gpk_allgatherv_* as ranks would — every line of the exchange but RCCL's own runs, with ranks that are apart in time.  Free the
 * communicators first, then the world. */
int32_t gpk_comm_mock_world(int32_t world, void** out_world);
int32_t gpk_comm_init_mock(int32_t rank, void* world, gpk_comm** out);
int32_t gpk_comm_mock_world_free(void* world);
int32_t gpk_allgatherv_geoarray(gpk_comm* comm, const gpk_geoarray* shard, void* stream, gpk_geoarray** out,
                                int64_t* out_row_base, int64_t* out_bytes);
int32_t gpk_allgatherv_rows_f64(gpk_comm* comm, const double* local_dev, int64_t n_local, int32_t width, double* out_dev,
                                int64_t out_capacity_rows, int64_t* out_total_rows, int64_t* out_counts, void* stream);

/* ---- join statistics (bench.py's edge_tests/s) ---------------------------------- */
/* While enabled, the point x polygonal join kernels count what their exact phase does (a few atomics per tile:
 * leave it off in timed regions).  out = {(point, part) pairs sent to the exact winding walk, edges walked for them,
 * left rows a chain-kernel join deferred to the generic walk (list cells, sub-cells without a chain entry, orientations
 * the floating-point filter could not certify), 0}, accumulated over the joins since the last reset; gpk_join_stats waits
 * for the device.  gpk_dwithin_join uses the last two words for its own counts: out[2] += bbox candidates, out[3] += candidates its
 * box-to-box test rejected before reading a coordinate (reset between joins of the two kinds to keep the meanings apart);
 * gpk_nearest_join_any counts the candidates of its search in the same two words. */
int32_t gpk_join_stats_enable(int32_t on);
int32_t gpk_join_stats(int64_t out[4], int32_t reset);

/* ---- profiling hooks (bench.py's roofline leg) -------------------------------------------- */
/* When enabled every kernel launch is bracketed by hipEvents on its stream. */
int32_t gpk_profile_enable(int32_t on);
/* Restrict the bracketing to kernels whose name contains `substr` (NULL or "" = every kernel).  Every event pair
 * drains the stream around its kernel (a few microseconds), so a timed region brackets only what it reports. */
int32_t gpk_profile_filter(const char* substr);
int32_t gpk_profile_reset(void);
/* accumulated milliseconds + launch count of kernels whose name contains `substr` */
int32_t gpk_profile_query(const char* substr, double* out_ms, int64_t* out_launches);

#ifdef __cplusplus
}
#endif
#endif /* GEOPOLARS_HIP_H */
