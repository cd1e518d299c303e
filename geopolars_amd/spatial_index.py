"""`SpatialIndex` / `spatial_join` — host-side mirror of geopolars/src/spatial_index.rs.

    SpatialJoinArgs         spatial_index.rs:15-35   (join_type, predicate, suffixes, prebuilt indexes)
    SpatialIndex            spatial_index.rs:314-350 (TryFrom<&Series>)
    spatial_join            spatial_index.rs:37-204
    spatial_join_nearest    GeoPandas' sjoin_nearest (not in the reference): every row — points, lines or polygons — with the nearest
                            geometries of another table (nearest_pairs for a POINT left column, nearest_pairs_any for the others)
    spatial_join_dwithin    GeoPandas' sjoin(predicate="dwithin", distance=d) (not in the reference): every pair within a distance
    spatial_join_relation   GeoPandas' sjoin(predicate=...) for lines x polygons (not in the reference): intersects, within, contains,
                            covers, covered_by, crosses, touches from the exact relation mask
    spatial_join_polygon_relation   the same for polygons x polygons: intersects, within, contains, covers, covered_by, touches,
                            overlaps, contains_properly, equals
    spatial_join_line_relation      the same for lines x lines: intersects, within, contains, covers, covered_by, crosses, touches,
                            overlaps, equals
    spatial_join_point_relation     the same with a point table on either side (or both): the nine names above from the point mask
    sjoin                           any two families: the one of the four relation joins that serves the pair
    spatial_join_intersection       polygons x polygons or lines x polygons (not in the reference): every pair that shares more than
                            a threshold of area / length, with the shared amount as an f64 `measure` column

The candidate generation + exact refine (spatial_index.rs:74-143) run on the GPU through
gpk_spatial_join; this module only marshals buffers and — for dataframe-shaped callers — assembles
the joined table from the (l, r) index pairs the way spatial_index.rs:145-203 does with polars
joins (here: pyarrow `take`, polars is not installed).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _abi
from ._abi import MEM_DEVICE, MEM_HOST, PREDICATES
from .geoarrow import DeviceGeoArray, GeoArrowArray
from .geoseries import (
    LINEAL,
    POLYGONAL,
    GeoSeries,
    _abi_name,
    _mismatch,
    dwithin_distance_arg,
    intersection_families_arg,
    intersection_min_measure_arg,
    line_clip_call,
    point_relation_sides,
    polygon_clip_call,
    predicate_route,
    relation_sides,
)


def _ptr(t):
    """data_ptr() of an optional torch tensor (None stays None: the ABI's "not asked for")"""
    return t.data_ptr() if t is not None else None


def _index_parts(for_points: bool, full: bool, light: bool) -> int:
    """the GPK_INDEX_* bits of gpk_index_build_ex"""
    parts = _abi.INDEX_BBOX_GRID | (_abi.INDEX_PIP if for_points else 0) | (_abi.INDEX_PIP_FULL if for_points and full else 0)
    if for_points and light and not full:  # an index that serves ONE join (what gpk_spatial_join builds for itself without r_index)
        parts |= _abi.INDEX_PIP_LIGHT
    return parts


class SpatialIndex:
    """Device-resident bbox grid directory over one series (the R-tree's replacement)."""

    def __init__(self, series: GeoSeries, stream: int = 0, for_points: bool = True, full: bool = False, light: bool = False):
        """for_points=False skips the point-in-polygon raster + edge slabs (only point x polygonal joins read them);
        full=True builds per-entry records for every list cell (GPK_INDEX_PIP_FULL: an index that serves hundreds of joins)."""
        self.series = series
        h = C.c_void_p()
        parts = _index_parts(for_points, full, light)
        _abi.check(_abi.lib().gpk_index_build_ex(series.device().handle, parts, None, stream, C.byref(h)))
        self._h = h

    @staticmethod
    def from_device(dev: DeviceGeoArray, stream: int = 0, for_points: bool = True, bboxes=None, full: bool = False, light: bool = False) -> "SpatialIndex":
        """Index over a device-resident array.  `bboxes`: optional (n, 4) float64 CUDA tensor of precomputed leaves
        (minx, miny, maxx, maxy per geometry, e.g. all-gathered from the ranks that own the shards)."""
        self = SpatialIndex.__new__(SpatialIndex)
        self.series = None
        self._dev = dev
        h = C.c_void_p()
        parts = _index_parts(for_points, full, light)
        _abi.check(_abi.lib().gpk_index_build_ex(dev.handle, parts, _ptr(bboxes), stream, C.byref(h)))
        self._h = h
        return self

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def nbytes(self) -> int:
        n = C.c_int64(0)
        _abi.check(_abi.lib().gpk_index_nbytes(self._h, C.byref(n)))
        return int(n.value)

    def describe(self) -> dict:
        """gpk_index_describe: which point-in-polygon tables the index carries (raster side, lean, chains, routing image)."""
        out = (C.c_int64 * 8)()
        _abi.check(_abi.lib().gpk_index_describe(self._h, out))
        return {"R": int(out[0]), "lean": bool(out[1]), "chains": bool(out[2]), "route": bool(out[3]), "list_heavy": bool(out[4])}

    def query_envelopes(self, boxes, mode: str = "contained", stream: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """gpk_index_query_envelope for a batch of query boxes ((n, 4): minx, miny, maxx, maxy): the (query, geometry index) pairs
        sorted by (query, index) and the per-query counts.  mode: "contained" (rstar locate_in_envelope) | "intersecting"
        (locate_in_envelope_intersecting); closed intervals (spatial_index.rs:383-393,422-429)."""
        lib = _abi.lib()
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 4))
        n = len(b)
        m = {"contained": _abi.QUERY_CONTAINED, "intersecting": _abi.QUERY_INTERSECTING}[mode]
        counts = np.zeros(n, dtype=np.uint32)
        n_pairs = C.c_int64(0)
        _abi.check(lib.gpk_index_query_envelope(self._h, b.ctypes.data, n, m, counts.ctypes.data, None, 0, C.byref(n_pairs), MEM_HOST, stream))
        pairs = np.zeros((int(n_pairs.value), 2), dtype=np.uint32)
        if len(pairs):
            _abi.check(lib.gpk_index_query_envelope(self._h, b.ctypes.data, n, m, counts.ctypes.data, pairs.ctypes.data, len(pairs), C.byref(n_pairs), MEM_HOST, stream))
        return pairs, counts

    def locate_in_envelope(self, lower, upper) -> np.ndarray:
        """`r_tree.locate_in_envelope(&AABB::from_corners(lower, upper))` (spatial_index.rs:383-387): the indexes of the geometries
        whose bounding box lies inside the closed query box, ascending."""
        pairs, _ = self.query_envelopes([[lower[0], lower[1], upper[0], upper[1]]], "contained")
        return pairs[:, 1].astype(np.int64)

    def locate_in_envelope_intersecting(self, lower, upper) -> np.ndarray:
        """rstar `locate_in_envelope_intersecting`: the geometries whose bounding box meets the closed query box."""
        pairs, _ = self.query_envelopes([[lower[0], lower[1], upper[0], upper[1]]], "intersecting")
        return pairs[:, 1].astype(np.int64)

    def free(self) -> None:
        if self._h:
            _abi.lib().gpk_index_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


@dataclass
class SpatialJoinArgs:
    """spatial_index.rs:15-35; defaults from `impl Default` (spatial_index.rs:24-35)."""

    join_type: str = "inner"  # JoinType::Inner | "left"
    predicate: str = "intersects"  # Predicate::Intersects
    l_suffix: Optional[str] = "_left"
    r_suffix: Optional[str] = "_right"
    l_index: Optional[SpatialIndex] = None  # accepted for signature parity; only the right index is used
    r_index: Optional[SpatialIndex] = None
    # not in the reference (its geometry columns are WKB, which names its type per row): the geometry type of a NATIVE GeoArrow column
    # whose nesting alone does not tell it — one list level is a LineString or a MultiPoint, two a Polygon or a MultiLineString — and
    # which carries no ARROW:extension:name (geoarrow.*).  spatial_join refuses such a column without a hint rather than guess.
    l_geom_type: int = -1
    r_geom_type: int = -1
    # how the geometry columns leave the join: "wkb" — as the reference holds them — or "geoarrow": native GeoArrow over Struct<x, y>,
    # gathered on the device (gpk_geoarray_take) from the series the join uploaded, without a detour through WKB
    geometry_encoding: str = "wkb"


GEOMETRY_ENCODINGS = ("wkb", "geoarrow")


def _pairs_with_retry(n: int, call, want_dist: bool = False, payload=np.float64):
    """The host-buffer joins' sizing loop: one call in the common case; the ABI reports the exact total when the capacity is too small.
    call(pairs_ptr, dist_ptr or None, capacity, byref(n_pairs)) makes the C call and returns its code.  Returns the pairs and — when
    asked for — their distances (or another per-pair payload of dtype `payload`), cut to the total."""
    n_pairs = C.c_int64(0)
    capacity = max(1024, 4 * n)
    while True:
        pairs = np.empty((capacity, 2), dtype=np.uint32)
        dist = np.empty(capacity, dtype=payload) if want_dist else None
        rc = call(pairs.ctypes.data, dist.ctypes.data if want_dist else None, capacity, C.byref(n_pairs))
        if rc == _abi.GPK_ERR_CAPACITY and int(n_pairs.value) > capacity:
            capacity = int(n_pairs.value)
            continue
        _abi.check(rc)
        h = int(n_pairs.value)
        return pairs[:h].copy(), (dist[:h].copy() if want_dist else None)


def join_pairs(
    left: GeoSeries,
    right: GeoSeries,
    predicate: str = "intersects",
    r_index: Optional[SpatialIndex] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray]:
    """All (l, r) index pairs with predicate(left[l], right[r]), sorted by (l, r), plus the per-left-row
    hit counts.  Host-buffer variant: sizes the pair buffer with a count-only first call."""
    lib = _abi.lib()
    n = len(left)
    counts = np.empty(n, dtype=np.uint32)
    rh = r_index.handle if r_index is not None else None
    pred = PREDICATES[predicate]
    call = lambda pairs_ptr, _dist, capacity, n_pairs: lib.gpk_spatial_join(  # noqa: E731
        left.device().handle, right.device().handle, rh, pred, left_row_base, counts.ctypes.data, pairs_ptr, capacity, n_pairs, MEM_HOST, None)
    return _pairs_with_retry(n, call)[0], counts


def join_pairs_device(left: DeviceGeoArray, right: DeviceGeoArray, r_index: SpatialIndex, predicate: str, out_counts, out_pairs, left_row_base: int = 0, stream: int = 0) -> int:
    """Device-buffer variant (bench / multi-GPU path): out_counts (n,) uint32-as-int32 and out_pairs
    (cap, 2) torch CUDA tensors are filled in place on `stream`; returns the number of pairs."""
    n_pairs = C.c_int64(0)
    rh, cap = r_index.handle if r_index is not None else None, out_pairs.shape[0] if out_pairs is not None else 0
    _abi.check(_abi.lib().gpk_spatial_join(
        left.handle, right.handle, rh, PREDICATES[predicate], left_row_base, _ptr(out_counts), _ptr(out_pairs), cap, C.byref(n_pairs), MEM_DEVICE, stream))
    return int(n_pairs.value)


def join_pairs_enqueue(left: DeviceGeoArray, right: DeviceGeoArray, r_index: SpatialIndex, predicate: str, out_counts, out_pairs, n_pairs_out, left_row_base: int = 0, stream: int = 0) -> None:
    """Stream-ordered variant of join_pairs_device (gpk_spatial_join_async): the join is enqueued on `stream` and
    this returns without waiting.  n_pairs_out: a 1-element int64 CUDA tensor that receives the total (read it
    after synchronising; pairs beyond out_pairs' capacity are dropped)."""
    cap = out_pairs.shape[0] if out_pairs is not None else 0
    _abi.check(_abi.lib().gpk_spatial_join_async(
        left.handle, right.handle, r_index.handle, PREDICATES[predicate], left_row_base, _ptr(out_counts), _ptr(out_pairs), cap, _ptr(n_pairs_out), stream))


JOIN_TYPES = {"inner": 0, "left": 1}  # GPK_JOIN_*


def join_indices(counts: np.ndarray, pairs: np.ndarray, join_type: str = "inner", left_row_base: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """(hit counts, sorted (l, r) pairs) -> i64 row indices (l, r) of the joined table (gpk_join_indices; the two
    u64 index Series of spatial_index.rs:147-159 followed by inner_join / left_join).  Left join: unmatched left
    rows appear once with r = -1."""
    lib = _abi.lib()
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n_rows = C.c_int64(0)
    jt = JOIN_TYPES[join_type]
    args = (counts.ctypes.data, pairs.ctypes.data if len(pairs) else None, len(counts), len(pairs), left_row_base, jt)
    _abi.check(lib.gpk_join_indices(*args, None, None, 0, C.byref(n_rows), MEM_HOST, None))
    n = int(n_rows.value)
    li, ri = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    if n:
        _abi.check(lib.gpk_join_indices(*args, li.ctypes.data, ri.ctypes.data, n, C.byref(n_rows), MEM_HOST, None))
    return li, ri


def take_column(column, idx: np.ndarray):
    """pyarrow column gathered by i64 row indices on the GPU (gpk_take_fixed / gpk_take_binary); -1 gives a null.
    Fixed-width primitives, booleans, binary and string columns — the types the reference's fixtures carry; anything
    else is reported (there is no host fallback)."""
    import pyarrow as pa

    lib = _abi.lib()
    arr = column.combine_chunks() if isinstance(column, pa.ChunkedArray) else column
    if arr.offset != 0:
        arr = pa.concat_arrays([arr])  # re-base a sliced array so the raw buffers start at row 0
    t = arr.type
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    n_idx, n = len(idx), len(arr)
    bufs = arr.buffers()
    validity = np.frombuffer(bufs[0], dtype=np.uint8) if bufs[0] is not None else None
    vptr = validity.ctypes.data if validity is not None else None
    out_valid = np.zeros((n_idx + 7) // 8, dtype=np.uint8)
    if pa.types.is_binary(t) or pa.types.is_string(t):
        offsets = np.frombuffer(bufs[1], dtype=np.int32)[: n + 1] if bufs[1] is not None else np.zeros(1, np.int32)
        values = np.frombuffer(bufs[2], dtype=np.uint8) if bufs[2] is not None and bufs[2].size else np.zeros(1, np.uint8)
        n_bytes = C.c_int64(0)
        out_off = np.zeros(n_idx + 1, dtype=np.int32)
        args = (values.ctypes.data, offsets.ctypes.data, vptr, n, idx.ctypes.data, n_idx, out_off.ctypes.data)
        _abi.check(lib.gpk_take_binary(*args, None, 0, C.byref(n_bytes), out_valid.ctypes.data, MEM_HOST, None))
        out_vals = np.empty(max(int(n_bytes.value), 1), dtype=np.uint8)
        if n_bytes.value:
            _abi.check(lib.gpk_take_binary(*args, out_vals.ctypes.data, int(n_bytes.value), C.byref(n_bytes), out_valid.ctypes.data, MEM_HOST, None))
        return pa.Array.from_buffers(t, n_idx, [pa.py_buffer(out_valid.tobytes()), pa.py_buffer(out_off.tobytes()), pa.py_buffer(out_vals[: int(n_bytes.value)].tobytes())])
    if pa.types.is_boolean(t):
        bits = 1
    elif pa.types.is_primitive(t):
        bits = t.bit_width
    else:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"join assembly: column type {t} is not supported")
    data = np.frombuffer(bufs[1], dtype=np.uint8) if bufs[1] is not None else np.zeros(16, np.uint8)
    out = np.zeros((n_idx + 7) // 8 if bits == 1 else n_idx * (bits // 8), dtype=np.uint8)
    _abi.check(lib.gpk_take_fixed(data.ctypes.data, bits, vptr, n, idx.ctypes.data, n_idx, out.ctypes.data if len(out) else None, out_valid.ctypes.data, MEM_HOST, None))
    return pa.Array.from_buffers(t, n_idx, [pa.py_buffer(out_valid.tobytes()), pa.py_buffer(out.tobytes())])


def _geometry_type_of(table, hint: int, hint_name: str) -> int:
    """the geom_type to import a table's geometry column with: the caller's hint, else -1 (WKB names its types; a GeoArrow extension
    name does; three list levels and bare coordinates can only be one type) — or an error for one / two list levels without either"""
    import pyarrow as pa

    if hint >= 0:
        return hint
    t = table.schema.field("geometry").type
    ext = (table.schema.field("geometry").metadata or {}).get(b"ARROW:extension:name")
    if isinstance(t, pa.BaseExtensionType):
        ext, t = t.extension_name.encode(), t.storage_type
    depth = 0
    while pa.types.is_list(t) or pa.types.is_large_list(t):
        depth, t = depth + 1, t.value_type
    if depth in (1, 2) and not ext:
        kinds = "LineString or MultiPoint" if depth == 1 else "Polygon or MultiLineString"
        raise _abi.GeopolarsHipError(
            _abi.GPK_ERR_INVALID_ARGUMENT,
            f"spatial_join: a GeoArrow geometry column of {depth} list level(s) without an ARROW:extension:name is a {kinds} column: "
            f"name the type in SpatialJoinArgs.{hint_name}",
        )
    return -1


def _as_wkb(column, geo: GeoSeries):
    """a native GeoArrow geometry column leaves a join the way the reference's geometry columns are held — WKB binary
    (from_geom_vec, util.rs:11-24) — encoded on the GPU from the series the join already uploaded"""
    import pyarrow as pa

    if pa.types.is_binary(column.type) or pa.types.is_large_binary(column.type):
        return column
    return geo.device().to_arrow("wkb")  # (gpk_geoarray_to_arrow: the library's buffers, validity included, released by pyarrow)


def _assemble(lhs, rhs, lgeo: GeoSeries, rgeo: GeoSeries, li: np.ndarray, ri: np.ndarray, l_suffix, r_suffix, distance_col=None, dist=None,
              geometry_encoding: str = "wkb"):
    """The joined table of spatial_index.rs:165-199 from the i64 row indices: suffixed left columns, suffixed right columns, then —
    for the distance joins — `distance_col` with each pair's distance (null for an unmatched left row).  geometry_encoding "geoarrow":
    the geometry columns are gathered as native GeoArrow on the device (a null row where r = -1) and exported over Struct<x, y>."""
    import pyarrow as pa

    cols, names = [], []
    for table, geo, idx, suffix in ((lhs, lgeo, li, l_suffix), (rhs, rgeo, ri, r_suffix)):
        for name in table.column_names:
            if name == "geometry" and geometry_encoding == "geoarrow":
                cols.append(geo.device().take(idx).to_arrow("struct"))
            else:
                cols.append(take_column(_as_wkb(table.column(name), geo) if name == "geometry" else table.column(name), idx))
            names.append(name + (suffix or ""))
    if distance_col is not None:
        # join_indices keeps the pairs' order and puts an unmatched left row (r = -1) where its pairs would be: pair k of the sorted
        # output is joined row k among the rows with r >= 0
        matched = ri >= 0
        d = np.zeros(len(ri), dtype=np.float64)
        d[matched] = dist
        cols.append(pa.array(d, type=pa.float64(), mask=~matched))
        names.append(distance_col)
    return pa.table(cols, names=names)


def spatial_join(lhs, rhs, options: Optional[SpatialJoinArgs] = None):
    """spatial_join(lhs, rhs, SpatialJoinArgs) over pyarrow Tables with a `geometry` column (spatial_index.rs:44-45) — WKB binary as the
    reference holds it, or a native GeoArrow nesting.  Returns a pyarrow Table shaped like the reference's result: suffixed left columns,
    then suffixed right columns (spatial_index.rs:165-199).  The geometry columns cross into the library the way every Series crosses
    the reference's FFI — as Arrow C Data Interface structs (py-geopolars/src/ffi.rs:12-32; gpk_geoarray_from_arrow): WKB is decoded
    on the GPU, nothing is rewritten on the host."""
    options = options or SpatialJoinArgs()
    if options.join_type not in ("inner", "left"):
        # spatial_index.rs:200-202 rejects every other JoinType
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, "Failed to generate the spatial index for the left dataframe")
    if options.geometry_encoding not in GEOMETRY_ENCODINGS:
        raise _abi.GeopolarsHipError(
            _abi.GPK_ERR_INVALID_ARGUMENT, f"spatial_join: geometry_encoding {options.geometry_encoding!r}: one of {', '.join(GEOMETRY_ENCODINGS)}")
    lgeo = GeoSeries.from_arrow(lhs.column("geometry"), _geometry_type_of(lhs, options.l_geom_type, "l_geom_type"))
    rgeo = GeoSeries.from_arrow(rhs.column("geometry"), _geometry_type_of(rhs, options.r_geom_type, "r_geom_type"))
    r_index = options.r_index or SpatialIndex(rgeo)
    pairs, counts = join_pairs(lgeo, rgeo, options.predicate, r_index)
    li, ri = join_indices(counts, pairs, options.join_type)  # i64 row indices, r = -1 for unmatched left rows
    return _assemble(lhs, rhs, lgeo, rgeo, li, ri, options.l_suffix, options.r_suffix, geometry_encoding=options.geometry_encoding)


# ---- nearest-neighbour join (gpk_nearest_join) ----------------------------------------------------------------------------------


@dataclass
class SpatialJoinNearestArgs:
    """Options of spatial_join_nearest (GeoPandas' sjoin_nearest over this module's table shape)."""

    join_type: str = "inner"  # "inner" | "left" (unmatched left rows once, with nulls on the right)
    max_distance: Optional[float] = None  # None: no limit; else only pairs with distance <= max_distance
    distance_col: Optional[str] = None  # name of a float64 column with each pair's distance (null for unmatched left rows)
    l_suffix: Optional[str] = "_left"
    r_suffix: Optional[str] = "_right"
    r_index: Optional[SpatialIndex] = None
    l_geom_type: int = -1  # as in SpatialJoinArgs
    r_geom_type: int = -1


def _max_distance_arg(max_distance: Optional[float]) -> float:
    """None -> INFINITY; a negative or NaN bound is refused here, before any device call"""
    if max_distance is None:
        return float("inf")
    d = float(max_distance)
    if not d >= 0.0:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"nearest join: max_distance must be >= 0 (None: no limit), got {max_distance!r}")
    return d


def _require_point_series(left: GeoSeries) -> None:
    """the left side of a nearest join holds points (checked on the series' own buffers: nothing is uploaded for it)"""
    t = left._array.geom_type if left._array is not None else left._dev.geom_type
    if t != _abi.GEOM_POINT:
        raise _abi.MismatchedGeometry(_abi.GPK_ERR_MISMATCHED_GEOMETRY, f"nearest join: the left side must be POINT (found type {t})")


def nearest_pairs(
    left: GeoSeries,
    right: GeoSeries,
    r_index: Optional[SpatialIndex] = None,
    max_distance: Optional[float] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """For every point of `left`, the rows of `right` at the smallest distance (ties all returned; within max_distance when given):
    (pairs (H, 2) uint32 sorted by (l, r), counts (n_left,) uint32, distances (H,) float64).  Host-buffer variant: the pair buffer
    is sized like join_pairs'."""
    md = _max_distance_arg(max_distance)
    _require_point_series(left)
    lib = _abi.lib()
    n = len(left)
    counts = np.empty(n, dtype=np.uint32)
    rh = r_index.handle if r_index is not None else None
    call = lambda pairs_ptr, dist_ptr, capacity, n_pairs: lib.gpk_nearest_join(  # noqa: E731
        left.device().handle, right.device().handle, rh, md, left_row_base, counts.ctypes.data, pairs_ptr, dist_ptr, capacity, n_pairs, MEM_HOST, None)
    pairs, dist = _pairs_with_retry(n, call, want_dist=True)
    return pairs, counts, dist


def nearest_pairs_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    out_counts,
    out_pairs,
    out_dist=None,
    max_distance: Optional[float] = None,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_dist (cap,) float64 torch CUDA tensors (any
    may be None; out_pairs None = count only) are filled in place on `stream`; returns the number of pairs."""
    md = _max_distance_arg(max_distance)
    if left.geom_type != _abi.GEOM_POINT:
        raise _abi.MismatchedGeometry(_abi.GPK_ERR_MISMATCHED_GEOMETRY, f"nearest join: the left side must be POINT (found type {left.geom_type})")
    n_pairs = C.c_int64(0)
    rh, cap = r_index.handle if r_index is not None else None, out_pairs.shape[0] if out_pairs is not None else 0
    _abi.check(_abi.lib().gpk_nearest_join(
        left.handle, right.handle, rh, md, left_row_base, _ptr(out_counts), _ptr(out_pairs), _ptr(out_dist), cap, C.byref(n_pairs), MEM_DEVICE, stream))
    return int(n_pairs.value)


NEAREST_FAMILIES = (_abi.GEOM_POINT, _abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON)


def _require_nearest_families(left_family: int, right_family: int) -> None:
    """both sides of gpk_nearest_join_any hold one of the six families (checked on the series' own type: nothing is uploaded for it)"""
    for side, t in (("left", left_family), ("right", right_family)):
        if t not in NEAREST_FAMILIES:
            raise _mismatch(f"nearest join: the {side} side must be Point, MultiPoint, LineString, MultiLineString, Polygon or MultiPolygon (found {_abi_name(t)})")


def nearest_pairs_any(
    left: GeoSeries,
    right: GeoSeries,
    r_index: Optional[SpatialIndex] = None,
    max_distance: Optional[float] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """nearest_pairs for any two geometry families (gpk_nearest_join_any): for every row of `left`, the rows of `right` at the smallest
    distance (ties all returned; within max_distance when given): (pairs (H, 2) uint32 sorted by (l, r), counts (n_left,) uint32,
    distances (H,) float64 — the doubles GeoSeries.distance returns for the pairs).  For a POINT `left` the result is nearest_pairs'.
    Host-buffer variant: the pair buffer is sized like join_pairs'."""
    md = _max_distance_arg(max_distance)
    _require_nearest_families(left._family(), right._family())
    return _payload_pairs("gpk_nearest_join_any", left, right, r_index, md, left_row_base)


def nearest_pairs_any_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    out_counts,
    out_pairs,
    out_dist=None,
    max_distance: Optional[float] = None,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_dist (cap,) float64 torch CUDA tensors (any
    may be None; out_pairs None = count only) are filled in place on `stream`; returns the number of pairs."""
    md = _max_distance_arg(max_distance)
    _require_nearest_families(left.geom_type, right.geom_type)
    return _payload_pairs_device("gpk_nearest_join_any", left, right, r_index, md, out_counts, out_pairs, out_dist, left_row_base, stream)


def spatial_join_nearest(lhs, rhs, options: Optional[SpatialJoinNearestArgs] = None):
    """GeoPandas' sjoin_nearest over pyarrow Tables with a `geometry` column (WKB or native GeoArrow, as spatial_join takes them): every
    left row with every right geometry at its smallest distance (ties all kept), shaped like spatial_join's result — suffixed left
    columns, suffixed right columns, then `distance_col` when asked for.  Any two of the six geometry families: a POINT left column goes
    through gpk_nearest_join, every other one through gpk_nearest_join_any."""
    options = options or SpatialJoinNearestArgs()
    if options.join_type not in ("inner", "left"):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"nearest join: join_type must be 'inner' or 'left', got {options.join_type!r}")
    md = _max_distance_arg(options.max_distance)
    lgeo = GeoSeries.from_arrow(lhs.column("geometry"), _geometry_type_of(lhs, options.l_geom_type, "l_geom_type"))
    rgeo = GeoSeries.from_arrow(rhs.column("geometry"), _geometry_type_of(rhs, options.r_geom_type, "r_geom_type"))
    if lgeo._family() == _abi.GEOM_POINT:
        pairs, counts, dist = nearest_pairs(lgeo, rgeo, options.r_index, md)
    else:
        pairs, counts, dist = nearest_pairs_any(lgeo, rgeo, options.r_index, md)
    li, ri = join_indices(counts, pairs, options.join_type)  # i64 row indices, r = -1 for unmatched left rows
    return _assemble(lhs, rhs, lgeo, rgeo, li, ri, options.l_suffix, options.r_suffix, options.distance_col, dist)


# ---- k-nearest-neighbours join (gpk_knn_join) -----------------------------------------------------------------------------------


@dataclass
class SpatialJoinKnnArgs:
    """Options of spatial_join_knn: every left row with its k nearest right rows, nearest first."""

    k: int = 1  # 1 .. GPK_KNN_MAX_K
    join_type: str = "inner"  # "inner" | "left" (unmatched left rows once, with nulls on the right)
    max_distance: Optional[float] = None  # None: no limit; else only pairs with distance <= max_distance
    exclude_self: bool = False  # never pair row i with row i (a table joined against itself)
    distance_col: Optional[str] = None  # name of a float64 column with each pair's distance (null for unmatched left rows)
    rank_col: Optional[str] = None  # name of a nullable uint32 column: 0 is the nearest (null for unmatched left rows)
    l_suffix: Optional[str] = "_left"
    r_suffix: Optional[str] = "_right"
    r_index: Optional[SpatialIndex] = None
    l_geom_type: int = -1  # as in SpatialJoinArgs
    r_geom_type: int = -1


def _knn_k_arg(k) -> int:
    """k of a knn join, refused here — before any device call — unless it is an integer in 1 .. GPK_KNN_MAX_K"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= _abi.GPK_KNN_MAX_K:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"knn join: k must be an integer in 1 .. {_abi.GPK_KNN_MAX_K}, got {k!r}")
    return int(k)


def knn_pairs(
    left: GeoSeries,
    right: GeoSeries,
    k: int,
    r_index: Optional[SpatialIndex] = None,
    max_distance: Optional[float] = None,
    exclude_self: bool = False,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """For every row of `left`, its k nearest rows of `right` (gpk_knn_join; any two geometry families; within max_distance when given;
    exclude_self: never row l + left_row_base itself): (pairs (H, 2) uint32 sorted by (l, distance, r), counts (n_left,) uint32, each at
    most k, distances (H,) float64 — the doubles GeoSeries.distance returns for the pairs).  A tie at the k-th place goes to the lower
    right row.  Host-buffer variant: the buffers hold n_left * k pairs, which always suffices."""
    k = _knn_k_arg(k)
    md = _max_distance_arg(max_distance)
    _require_nearest_families(left._family(), right._family())
    n = len(left)
    capacity = max(1, n * k)
    counts = np.zeros(n, dtype=np.uint32)
    pairs, dist = np.empty((capacity, 2), dtype=np.uint32), np.empty(capacity, dtype=np.float64)
    n_pairs = C.c_int64(0)
    _abi.check(_abi.lib().gpk_knn_join(
        left.device().handle, right.device().handle, r_index.handle if r_index is not None else None, k, md,
        _abi.GPK_KNN_EXCLUDE_SELF if exclude_self else 0, left_row_base, counts.ctypes.data, pairs.ctypes.data, dist.ctypes.data, capacity,
        C.byref(n_pairs), MEM_HOST, None))
    h = int(n_pairs.value)
    return pairs[:h].copy(), counts, dist[:h].copy()


def knn_pairs_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    k: int,
    out_counts,
    out_pairs,
    out_dist=None,
    max_distance: Optional[float] = None,
    exclude_self: bool = False,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_dist (cap,) float64 torch CUDA tensors (any
    may be None; out_pairs None = count only) are filled in place on `stream`; returns the number of pairs."""
    k = _knn_k_arg(k)
    md = _max_distance_arg(max_distance)
    _require_nearest_families(left.geom_type, right.geom_type)
    n_pairs = C.c_int64(0)
    rh, cap = r_index.handle if r_index is not None else None, out_pairs.shape[0] if out_pairs is not None else 0
    _abi.check(_abi.lib().gpk_knn_join(
        left.handle, right.handle, rh, k, md, _abi.GPK_KNN_EXCLUDE_SELF if exclude_self else 0, left_row_base, _ptr(out_counts), _ptr(out_pairs),
        _ptr(out_dist), cap, C.byref(n_pairs), MEM_DEVICE, stream))
    return int(n_pairs.value)


def spatial_join_knn(lhs, rhs, options: Optional[SpatialJoinKnnArgs] = None):
    """The k-nearest-neighbours join over pyarrow Tables with a `geometry` column (WKB or native GeoArrow, as spatial_join takes them):
    every left row with its k nearest right geometries, nearest first, shaped like spatial_join's result — suffixed left columns,
    suffixed right columns, then `distance_col` and `rank_col` when asked for.  Any two of the six geometry families."""
    options = options or SpatialJoinKnnArgs()
    if options.join_type not in ("inner", "left"):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"knn join: join_type must be 'inner' or 'left', got {options.join_type!r}")
    k = _knn_k_arg(options.k)
    md = _max_distance_arg(options.max_distance)
    lgeo = GeoSeries.from_arrow(lhs.column("geometry"), _geometry_type_of(lhs, options.l_geom_type, "l_geom_type"))
    rgeo = GeoSeries.from_arrow(rhs.column("geometry"), _geometry_type_of(rhs, options.r_geom_type, "r_geom_type"))
    pairs, counts, dist = knn_pairs(lgeo, rgeo, k, options.r_index, md, options.exclude_self)
    li, ri = join_indices(counts, pairs, options.join_type)  # i64 row indices, r = -1 for unmatched left rows
    table = _assemble(lhs, rhs, lgeo, rgeo, li, ri, options.l_suffix, options.r_suffix, options.distance_col, dist)
    if options.rank_col is not None:
        import pyarrow as pa

        # pair j of a left row has rank j: the pairs come nearest first
        starts = np.concatenate([[0], np.cumsum(counts.astype(np.int64))[:-1]]) if len(counts) else np.zeros(0, np.int64)
        rank = (np.arange(len(pairs), dtype=np.int64) - np.repeat(starts, counts.astype(np.int64))).astype(np.uint32)
        matched = ri >= 0
        rk = np.zeros(len(ri), dtype=np.uint32)
        rk[matched] = rank
        table = table.append_column(options.rank_col, pa.array(rk, type=pa.uint32(), mask=~matched))
    return table


# ---- what the joins with a value per pair share (dwithin, the three relation joins, the intersection measure) --------------------------
# Their ABI calls have one shape: (left, right, index, <one family argument>, left_row_base, counts, pairs, payload, capacity, n_pairs,
# space, stream).  The public functions below validate their own argument, then go through these.


def _payload_pairs(abi_name: str, left: GeoSeries, right: GeoSeries, r_index: Optional[SpatialIndex], arg, left_row_base: int, payload=np.float64):
    """host buffers: (pairs, counts, per-pair payload of dtype `payload`), the pair buffer sized like join_pairs'"""
    fn = getattr(_abi.lib(), abi_name)
    n = len(left)
    counts = np.zeros(n, dtype=np.uint32)
    rh = r_index.handle if r_index is not None else None
    call = lambda pairs_ptr, payload_ptr, capacity, n_pairs: fn(  # noqa: E731
        left.device().handle, right.device().handle, rh, arg, left_row_base, counts.ctypes.data, pairs_ptr, payload_ptr, capacity, n_pairs, MEM_HOST, None)
    pairs, values = _pairs_with_retry(n, call, want_dist=True, payload=payload)
    return pairs, counts, values


def _payload_pairs_device(abi_name: str, left: DeviceGeoArray, right: DeviceGeoArray, r_index: Optional[SpatialIndex], arg, out_counts, out_pairs,
                          out_payload, left_row_base: int, stream: int) -> int:
    """device buffers, filled in place on `stream`: the number of pairs"""
    n_pairs = C.c_int64(0)
    rh, cap = r_index.handle if r_index is not None else None, out_pairs.shape[0] if out_pairs is not None else 0
    _abi.check(getattr(_abi.lib(), abi_name)(
        left.handle, right.handle, rh, arg, left_row_base, _ptr(out_counts), _ptr(out_pairs), _ptr(out_payload), cap, C.byref(n_pairs), MEM_DEVICE, stream))
    return int(n_pairs.value)


def _payload_table_join(what: str, lhs, rhs, options, family_arg, pairs_fn, value_col: Optional[str] = None, relation_col: Optional[str] = None):
    """The table joins over `pairs_fn(left, right, arg, r_index)`: `what` prefixes the join_type message, `family_arg()` checks the
    family's own options (before a geometry column is decoded) and returns the argument.  The payload becomes the float64 `value_col`
    or the nullable uint8 `relation_col` (null for an unmatched left row)."""
    if options.join_type not in ("inner", "left"):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{what}: join_type must be 'inner' or 'left', got {options.join_type!r}")
    arg = family_arg()
    lgeo = GeoSeries.from_arrow(lhs.column("geometry"), _geometry_type_of(lhs, options.l_geom_type, "l_geom_type"))
    rgeo = GeoSeries.from_arrow(rhs.column("geometry"), _geometry_type_of(rhs, options.r_geom_type, "r_geom_type"))
    pairs, counts, values = pairs_fn(lgeo, rgeo, arg, options.r_index)
    li, ri = join_indices(counts, pairs, options.join_type)  # i64 row indices, r = -1 for unmatched left rows
    table = _assemble(lhs, rhs, lgeo, rgeo, li, ri, options.l_suffix, options.r_suffix, value_col, values)
    if relation_col is not None:
        import pyarrow as pa

        matched = ri >= 0
        m = np.zeros(len(ri), dtype=np.uint8)
        m[matched] = values
        table = table.append_column(relation_col, pa.array(m, type=pa.uint8(), mask=~matched))
    return table


def _known_predicate(what: str, predicate: str, table: dict) -> str:
    if predicate not in table:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{what}: unknown predicate {predicate!r}: one of {sorted(table)}")
    return predicate


# ---- within-distance join (gpk_dwithin_join) ------------------------------------------------------------------------------------


@dataclass
class SpatialJoinDWithinArgs:
    """Options of spatial_join_dwithin (GeoPandas' sjoin(predicate="dwithin", distance=...) over this module's table shape)."""

    distance: Optional[float] = None  # required: finite and >= 0; pairs with distance(l, r) <= distance are joined
    join_type: str = "inner"  # "inner" | "left" (unmatched left rows once, with nulls on the right)
    distance_col: Optional[str] = None  # name of a float64 column with each pair's distance (null for unmatched left rows)
    l_suffix: Optional[str] = "_left"
    r_suffix: Optional[str] = "_right"
    r_index: Optional[SpatialIndex] = None
    l_geom_type: int = -1  # as in SpatialJoinArgs
    r_geom_type: int = -1


def dwithin_pairs(
    left: GeoSeries,
    right: GeoSeries,
    distance: float,
    r_index: Optional[SpatialIndex] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every (l, r) with distance(left[l], right[r]) <= `distance`, any two geometry families: (pairs (H, 2) uint32 sorted by (l, r),
    counts (n_left,) uint32, distances (H,) float64 — the doubles GeoSeries.distance returns for the pairs).  Host-buffer variant: the
    pair buffer is sized like join_pairs'."""
    d = dwithin_distance_arg(distance)
    return _payload_pairs("gpk_dwithin_join", left, right, r_index, d, left_row_base)


def dwithin_pairs_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    distance: float,
    out_counts,
    out_pairs,
    out_dist=None,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_dist (cap,) float64 torch CUDA tensors (any
    may be None; out_pairs None = count only) are filled in place on `stream`; returns the number of pairs."""
    d = dwithin_distance_arg(distance)
    return _payload_pairs_device("gpk_dwithin_join", left, right, r_index, d, out_counts, out_pairs, out_dist, left_row_base, stream)


def spatial_join_dwithin(lhs, rhs, options: Optional[SpatialJoinDWithinArgs] = None):
    """GeoPandas' sjoin(predicate="dwithin", distance=d) over pyarrow Tables with a `geometry` column (WKB or native GeoArrow, as
    spatial_join takes them): every left row with every right row within `options.distance` of it, shaped like spatial_join's result —
    suffixed left columns, suffixed right columns, then `distance_col` when asked for.  Any two geometry families."""
    options = options or SpatialJoinDWithinArgs()
    return _payload_table_join("dwithin join", lhs, rhs, options, lambda: dwithin_distance_arg(options.distance), dwithin_pairs, value_col=options.distance_col)


# ---- line x polygon predicate join (gpk_line_polygon_join) ----------------------------------------------------------------------

# GeoPandas' predicate names -> (GPK_LP_PRED_*, the side that must hold the lines: "left", "right" or None for either)
RELATION_PREDICATES = {
    "intersects": (_abi.LP_PRED_INTERSECTS, None),
    "crosses": (_abi.LP_PRED_CROSSES, None),
    "touches": (_abi.LP_PRED_TOUCHES, None),
    "within": (_abi.LP_PRED_WITHIN, "left"),
    "covered_by": (_abi.LP_PRED_COVERED_BY, "left"),
    "contains": (_abi.LP_PRED_WITHIN, "right"),
    "covers": (_abi.LP_PRED_COVERED_BY, "right"),
}


def relation_predicate_arg(predicate: str, left_family: int, right_family: int) -> int:
    """The GPK_LP_PRED_* id of a GeoPandas predicate name for a join of these two families, checked before any device call: one
    side lineal and the other polygonal, and the name must fit the side that holds the lines (`within` and `covered_by` say it of
    the left rows, so the lines are on the left; `contains` and `covers` need the polygons there)."""
    if predicate not in RELATION_PREDICATES:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"relation join: unknown predicate {predicate!r}: one of {sorted(RELATION_PREDICATES)}")
    line_left = relation_sides("relation join", left_family, right_family)
    pred, side = RELATION_PREDICATES[predicate]
    if side is not None and (side == "left") != line_left:
        raise _abi.GeopolarsHipError(
            _abi.GPK_ERR_INVALID_ARGUMENT,
            f"relation join: {predicate!r} needs the {'lines' if side == 'left' else 'polygons'} on the left (a line {'covers' if predicate in ('contains', 'covers') else 'lies within'} no polygon)",
        )
    return pred


@dataclass
class SpatialJoinRelationArgs:
    """Options of spatial_join_relation (GeoPandas' sjoin(predicate=...) for a lines table and a polygons table)."""

    predicate: str = "intersects"  # intersects | within | contains | covers | covered_by | crosses | touches
    join_type: str = "inner"  # "inner" | "left" (unmatched left rows once, with nulls on the right)
    relation_col: Optional[str] = None  # name of a uint8 column with each pair's relation mask (null for unmatched left rows)
    l_suffix: Optional[str] = "_left"
    r_suffix: Optional[str] = "_right"
    r_index: Optional[SpatialIndex] = None
    l_geom_type: int = -1  # as in SpatialJoinArgs
    r_geom_type: int = -1


def relation_pairs(
    left: GeoSeries,
    right: GeoSeries,
    predicate: str = "intersects",
    r_index: Optional[SpatialIndex] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every (l, r) of a lines column and a polygons column (either order) whose exact relation satisfies `predicate`: (pairs (H, 2)
    uint32 sorted by (l, r), counts (n_left,) uint32, masks (H,) uint8 — what GeoSeries.line_polygon_relation gives for the pairs).
    Host-buffer variant: the pair buffer is sized like join_pairs'."""
    pred = relation_predicate_arg(predicate, left._family(), right._family())
    return _payload_pairs("gpk_line_polygon_join", left, right, r_index, pred, left_row_base, payload=np.uint8)


def relation_pairs_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    predicate: str,
    out_counts,
    out_pairs,
    out_mask=None,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_mask (cap,) uint8 torch CUDA tensors (any may
    be None; out_pairs None = count only; without out_mask a pair's walk ends as soon as its predicate is settled) are filled in place
    on `stream`; returns the number of pairs."""
    pred = relation_predicate_arg(predicate, left.geom_type, right.geom_type)
    return _payload_pairs_device("gpk_line_polygon_join", left, right, r_index, pred, out_counts, out_pairs, out_mask, left_row_base, stream)


def spatial_join_relation(lhs, rhs, options: Optional[SpatialJoinRelationArgs] = None):
    """GeoPandas' sjoin(predicate=...) over two pyarrow Tables with a `geometry` column (WKB or native GeoArrow, as spatial_join takes
    them), one of lines and one of polygons: every left row with every right row in the relation, shaped like spatial_join's result —
    suffixed left columns, suffixed right columns, then `relation_col` (the pair's mask) when asked for."""
    options = options or SpatialJoinRelationArgs()
    return _payload_table_join("relation join", lhs, rhs, options, lambda: _known_predicate("relation join", options.predicate, RELATION_PREDICATES), relation_pairs,
                               relation_col=options.relation_col)


# ---- polygon x polygon predicate join (gpk_polygon_relation_join) ---------------------------------------------------------------

# GeoPandas' predicate names (plus `equals`) -> GPK_PP_PRED_*; for two areas covered_by is within and covers is contains
POLYGON_RELATION_PREDICATES = {
    "intersects": _abi.PP_PRED_INTERSECTS,
    "within": _abi.PP_PRED_WITHIN,
    "covered_by": _abi.PP_PRED_WITHIN,
    "contains": _abi.PP_PRED_CONTAINS,
    "covers": _abi.PP_PRED_CONTAINS,
    "touches": _abi.PP_PRED_TOUCHES,
    "overlaps": _abi.PP_PRED_OVERLAPS,
    "contains_properly": _abi.PP_PRED_CONTAINS_PROPERLY,
    "equals": _abi.PP_PRED_EQUALS,
}


def polygon_relation_predicate_arg(predicate: str, left_family: int, right_family: int) -> int:
    """The GPK_PP_PRED_* id of a predicate name for a join of these two families, checked before any device call: a known name and
    both sides polygonal.  The relation is always read "left row <predicate> right row"."""
    if predicate not in POLYGON_RELATION_PREDICATES:
        raise _abi.GeopolarsHipError(
            _abi.GPK_ERR_INVALID_ARGUMENT, f"polygon relation join: unknown predicate {predicate!r}: one of {sorted(POLYGON_RELATION_PREDICATES)}"
        )
    if left_family not in POLYGONAL or right_family not in POLYGONAL:
        raise _mismatch(
            f"polygon relation join: Polygon | MultiPolygon x Polygon | MultiPolygon (found {_abi_name(left_family)} x {_abi_name(right_family)})"
        )
    return POLYGON_RELATION_PREDICATES[predicate]


def polygon_relation_pairs(
    left: GeoSeries,
    right: GeoSeries,
    predicate: str = "intersects",
    r_index: Optional[SpatialIndex] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every (l, r) of two polygon columns (which may be the same column: adjacency, duplicates) whose exact relation satisfies
    `predicate`: (pairs (H, 2) uint32 sorted by (l, r), counts (n_left,) uint32, masks (H,) uint8 — what
    left.polygon_relation(right) gives for the pairs).  Host-buffer variant: the pair buffer is sized like join_pairs'."""
    pred = polygon_relation_predicate_arg(predicate, left._family(), right._family())
    return _payload_pairs("gpk_polygon_relation_join", left, right, r_index, pred, left_row_base, payload=np.uint8)


def polygon_relation_pairs_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    predicate: str,
    out_counts,
    out_pairs,
    out_mask=None,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_mask (cap,) uint8 torch CUDA tensors (any may
    be None; out_pairs None = count only; without out_mask the work on a pair ends as soon as its predicate is settled) are filled in
    place on `stream`; returns the number of pairs."""
    pred = polygon_relation_predicate_arg(predicate, left.geom_type, right.geom_type)
    return _payload_pairs_device("gpk_polygon_relation_join", left, right, r_index, pred, out_counts, out_pairs, out_mask, left_row_base, stream)


def spatial_join_polygon_relation(lhs, rhs, options: Optional[SpatialJoinRelationArgs] = None):
    """GeoPandas' sjoin(predicate=...) over two pyarrow Tables of polygons with a `geometry` column (WKB or native GeoArrow, as
    spatial_join takes them): every left row with every right row in the relation, shaped like spatial_join_relation's result —
    suffixed left columns, suffixed right columns, then `relation_col` (the pair's 4-bit mask) when asked for."""
    options = options or SpatialJoinRelationArgs()
    return _payload_table_join("polygon relation join", lhs, rhs, options, lambda: _known_predicate("polygon relation join", options.predicate, POLYGON_RELATION_PREDICATES), polygon_relation_pairs,
                               relation_col=options.relation_col)


# ---- intersection measure join (gpk_intersection_measure_join) --------------------------------------------------------------------


@dataclass
class SpatialJoinIntersectionArgs:
    """Options of spatial_join_intersection (an overlay's pair list with its weights: areal interpolation, IoU, length per zone)."""

    min_measure: float = 0.0  # finite and >= 0; pairs that share MORE than this are joined (at 0 a touching pair may appear at rounding level)
    join_type: str = "inner"  # "inner" | "left" (unmatched left rows once, with nulls on the right)
    measure_col: str = "measure"  # name of the float64 column with each pair's shared area / length (null for unmatched left rows)
    l_suffix: Optional[str] = "_left"
    r_suffix: Optional[str] = "_right"
    r_index: Optional[SpatialIndex] = None
    l_geom_type: int = -1  # as in SpatialJoinArgs
    r_geom_type: int = -1


def intersection_measure_pairs(
    left: GeoSeries,
    right: GeoSeries,
    min_measure: float = 0.0,
    r_index: Optional[SpatialIndex] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every (l, r) of a polygon column (the shared area) or a line column (the length inside) against a polygon column that share more
    than `min_measure`: (pairs (H, 2) uint32 sorted by (l, r), counts (n_left,) uint32, measures (H,) float64 — bit for bit what
    left.intersection_area(right) / left.intersection_length(right) gives for the pairs).  Host-buffer variant: the pair buffer is
    sized like join_pairs'."""
    m = intersection_min_measure_arg(min_measure)
    intersection_families_arg("intersection measure join", left._family(), right._family())
    return _payload_pairs("gpk_intersection_measure_join", left, right, r_index, m, left_row_base)


def intersection_measure_pairs_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    min_measure: float,
    out_counts,
    out_pairs,
    out_measure=None,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_measure (cap,) float64 torch CUDA tensors (any
    may be None; out_pairs None = count only) are filled in place on `stream`; returns the number of pairs."""
    m = intersection_min_measure_arg(min_measure)
    intersection_families_arg("intersection measure join", left.geom_type, right.geom_type)
    return _payload_pairs_device("gpk_intersection_measure_join", left, right, r_index, m, out_counts, out_pairs, out_measure, left_row_base, stream)


def spatial_join_intersection(lhs, rhs, options: Optional[SpatialJoinIntersectionArgs] = None):
    """The pair list of an overlay with its weights, over two pyarrow Tables with a `geometry` column (WKB or native GeoArrow, as
    spatial_join takes them): polygons or lines on the left, polygons on the right; every left row with every right row it shares more
    than `options.min_measure` of area (polygons) or length (lines) with, shaped like spatial_join's result — suffixed left columns,
    suffixed right columns, then the float64 `measure_col`."""
    options = options or SpatialJoinIntersectionArgs()

    def family_arg() -> float:
        if not isinstance(options.measure_col, str) or not options.measure_col:
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"intersection join: measure_col must be a column name, got {options.measure_col!r}")
        return intersection_min_measure_arg(options.min_measure)

    return _payload_table_join("intersection join", lhs, rhs, options, family_arg, intersection_measure_pairs, value_col=options.measure_col)


# ---- clip lines to polygons over a pair list (gpk_line_clip) ------------------------------------------------------------------------

CLIP_MODES = {"intersection": _abi.CLIP_INSIDE, "difference": _abi.CLIP_OUTSIDE}


def line_clip_mode_arg(how: str, lines_family: int, polys_family: int) -> int:
    """The GPK_CLIP_* mode of `how`, checked before any device call together with the families: lines x polygons, in that order."""
    if how not in CLIP_MODES:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"line clip: unknown how {how!r}: one of {sorted(CLIP_MODES)}")
    if lines_family not in LINEAL or polys_family not in POLYGONAL:
        swap = ": the lines come first, swap the arguments" if lines_family in POLYGONAL and polys_family in LINEAL else ""
        raise _mismatch(
            f"line clip: LineString | MultiLineString x Polygon | MultiPolygon (found {_abi_name(lines_family)} x {_abi_name(polys_family)}){swap}; "
            "the other families have intersection_area / intersection_length, not the geometry"
        )
    return CLIP_MODES[how]


def line_clip_pairs(lines: GeoSeries, polys: GeoSeries, l_idx, r_idx, how: str = "intersection", drop_empty: bool = False):
    """clip(lines[l_idx[k]], polys[r_idx[k]]) for every pair k, as a MULTILINESTRING GeoSeries (gpk_line_clip): what
    lines.intersection / difference gives row-wise, over an explicit pair list.  An index past the end of its column gives a null row.
    With `drop_empty` the rows without parts and the null rows are left out and the result is (series, src), src[k] (int32) = the pair
    of output row k."""
    mode = line_clip_mode_arg(how, lines._family(), polys._family())
    try:
        li, ri = np.ascontiguousarray(l_idx, dtype=np.uint32), np.ascontiguousarray(r_idx, dtype=np.uint32)
    except (TypeError, ValueError, OverflowError):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, "line clip: the pair lists must be arrays of row numbers") from None
    if li.ndim != 1 or li.shape != ri.shape:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"line clip: {li.size} line rows for {ri.size} polygon rows")
    n = len(li)
    src = np.empty(n, dtype=np.int32) if drop_empty else None
    if n == 0:  # (no pair, no call: a NULL list would mean the identity)
        z = np.zeros(1, dtype=np.int32)
        out = GeoSeries(GeoArrowArray(_abi.GEOM_MULTILINESTRING, np.zeros((0, 2)), geom_offsets=z, ring_offsets=z.copy(), n_geoms=0))
    else:
        out = line_clip_call(lines.device(), polys.device(), li.ctypes.data, ri.ctypes.data, n, MEM_HOST, mode,
                             _abi.CLIP_DROP_EMPTY if drop_empty else 0, src.ctypes.data if drop_empty else None, MEM_HOST)
    return (out, src[: len(out)]) if drop_empty else out


def line_clip_pairs_device(lines: DeviceGeoArray, polys: DeviceGeoArray, l_idx, r_idx, how: str = "intersection", drop_empty: bool = False,
                           out_src=None, stream: int = 0) -> GeoSeries:
    """Device-buffer variant: l_idx, r_idx (n,) uint32-as-int32 torch CUDA tensors (at least one row; None = the identity over that
    column), out_src an optional (n,) int32 CUDA tensor for the map of `drop_empty`; enqueued on `stream`.  Returns the series."""
    mode = line_clip_mode_arg(how, lines.geom_type, polys.geom_type)
    n = l_idx.shape[0] if l_idx is not None else (r_idx.shape[0] if r_idx is not None else lines.n_geoms)
    return line_clip_call(lines, polys, _ptr(l_idx), _ptr(r_idx), n, MEM_DEVICE, mode, _abi.CLIP_DROP_EMPTY if drop_empty else 0, _ptr(out_src),
                          MEM_DEVICE, stream)


@dataclass
class SpatialJoinClipArgs:
    """Options of spatial_join_clip."""

    r_index: Optional[SpatialIndex] = None  # an index of `right` carrying the bbox grid


def spatial_join_clip(left: GeoSeries, right: GeoSeries, args: Optional[SpatialJoinClipArgs] = None):
    """GeoPandas' overlay(lines, polys, how="intersection", keep_geom_type=True) as a pair list: gpk_line_polygon_join(intersects),
    then gpk_line_clip over the returned pairs, empty results dropped.  Either side may hold the lines.  Returns (l, r, geometry):
    int64 row numbers of `left` and `right`, sorted by (l, r), for the pairs that share a piece of positive length, and that piece of
    the LINE as a MULTILINESTRING GeoSeries — a pair that only touches is in the join and not here."""
    args = args or SpatialJoinClipArgs()
    line_left = relation_sides("clip join", left._family(), right._family())
    pairs, _counts, _masks = relation_pairs(left, right, "intersects", args.r_index)
    lines, polys = (left, right) if line_left else (right, left)
    li, pi = (pairs[:, 0], pairs[:, 1]) if line_left else (pairs[:, 1], pairs[:, 0])
    geometry, src = line_clip_pairs(lines, polys, li, pi, "intersection", drop_empty=True)
    kept = pairs[src]
    return kept[:, 0].astype(np.int64), kept[:, 1].astype(np.int64), geometry


# ---- polygon x polygon intersection and difference over a pair list (gpk_polygon_clip) ---------------------------------------------------

PCLIP_MODES = {"intersection": _abi.PCLIP_INTERSECTION, "difference": _abi.PCLIP_DIFFERENCE}


def polygon_clip_mode_arg(how: str, a_family: int, b_family: int) -> int:
    """The GPK_PCLIP_* mode of `how`, checked before any device call together with the families: polygons x polygons."""
    if how not in PCLIP_MODES:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"polygon clip: unknown how {how!r}: one of {sorted(PCLIP_MODES)}")
    if a_family not in POLYGONAL or b_family not in POLYGONAL:
        raise _mismatch(f"polygon clip: Polygon | MultiPolygon x Polygon | MultiPolygon (found {_abi_name(a_family)} x {_abi_name(b_family)})")
    return PCLIP_MODES[how]


def polygon_clip_pairs(a: GeoSeries, b: GeoSeries, l_idx, r_idx, how: str = "intersection", drop_empty: bool = False, return_status: bool = False):
    """clip(a[l_idx[k]], b[r_idx[k]]) for every pair k, as a MULTIPOLYGON GeoSeries (gpk_polygon_clip): what a.polygon_intersection /
    polygon_difference gives row-wise, over an explicit pair list.  An index past the end of its column gives a null row.  With
    `drop_empty` the rows without parts and the null rows are left out and src (int32), the pair of every output row, is returned as
    well; with `return_status` the uint8 status of every PAIR.  Returns the series, or (series[, src][, status])."""
    mode = polygon_clip_mode_arg(how, a._family(), b._family())
    return _polygon_pairs("gpk_polygon_clip", mode, a, b, l_idx, r_idx, drop_empty, return_status)


def _polygon_pairs(entry: str, mode: int, a: GeoSeries, b: GeoSeries, l_idx, r_idx, drop_empty: bool, return_status: bool):
    """polygon_clip_pairs / polygon_union_pairs / polygon_symdiff_pairs once the mode and the families are checked"""
    label = {"gpk_polygon_clip": "polygon clip", "gpk_polygon_union": "polygon union"}.get(entry, "polygon symmetric difference")
    try:
        li, ri = np.ascontiguousarray(l_idx, dtype=np.uint32), np.ascontiguousarray(r_idx, dtype=np.uint32)
    except (TypeError, ValueError, OverflowError):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{label}: the pair lists must be arrays of row numbers") from None
    if li.ndim != 1 or li.shape != ri.shape:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{label}: {li.size} rows of a for {ri.size} rows of b")
    n = len(li)
    src = np.empty(n, dtype=np.int32) if drop_empty else None
    status = np.empty(n, dtype=np.uint8) if return_status else None
    if n == 0:  # (no pair, no call: a NULL list would mean the identity)
        z = np.zeros(1, dtype=np.int32)
        out = GeoSeries(GeoArrowArray(_abi.GEOM_MULTIPOLYGON, np.zeros((0, 2)), geom_offsets=z, part_offsets=z.copy(), ring_offsets=z.copy(), n_geoms=0))
    else:
        out = polygon_clip_call(a.device(), b.device(), li.ctypes.data, ri.ctypes.data, n, MEM_HOST, mode, _abi.CLIP_DROP_EMPTY if drop_empty else 0,
                                src.ctypes.data if drop_empty else None, MEM_HOST, status.ctypes.data if return_status else None, MEM_HOST, entry=entry)
    res = (out,) + ((src[: len(out)],) if drop_empty else ()) + ((status,) if return_status else ())
    return res if len(res) > 1 else out


def polygon_clip_pairs_device(a: DeviceGeoArray, b: DeviceGeoArray, l_idx, r_idx, how: str = "intersection", drop_empty: bool = False,
                              out_src=None, out_status=None, stream: int = 0) -> GeoSeries:
    """Device-buffer variant: l_idx, r_idx (n,) uint32-as-int32 torch CUDA tensors (at least one row; None = the identity over that
    column), out_src an optional (n,) int32 CUDA tensor for the map of `drop_empty`, out_status an optional (n,) uint8 CUDA tensor;
    enqueued on `stream`.  Returns the series."""
    mode = polygon_clip_mode_arg(how, a.geom_type, b.geom_type)
    n = l_idx.shape[0] if l_idx is not None else (r_idx.shape[0] if r_idx is not None else a.n_geoms)
    return polygon_clip_call(a, b, _ptr(l_idx), _ptr(r_idx), n, MEM_DEVICE, mode, _abi.CLIP_DROP_EMPTY if drop_empty else 0, _ptr(out_src),
                             MEM_DEVICE, _ptr(out_status), MEM_DEVICE, stream)


# ---- polygon x polygon union over a pair list (gpk_polygon_union) ---------------------------------------------------------------------

PUNION_MODES = {"union": _abi.PUNION_UNION}


def polygon_union_mode_arg(how: str, a_family: int, b_family: int) -> int:
    """The GPK_PUNION_* mode of `how`, checked before any device call together with the families: polygons x polygons."""
    if how not in PUNION_MODES:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"polygon union: unknown how {how!r}: one of {sorted(PUNION_MODES)}")
    if a_family not in POLYGONAL or b_family not in POLYGONAL:
        raise _mismatch(f"polygon union: Polygon | MultiPolygon x Polygon | MultiPolygon (found {_abi_name(a_family)} x {_abi_name(b_family)})")
    return PUNION_MODES[how]


def polygon_union_pairs(a: GeoSeries, b: GeoSeries, a_rows, b_rows, how: str = "union", drop_empty: bool = False, return_status: bool = False):
    """union(a[a_rows[k]], b[b_rows[k]]) for every pair k, as a MULTIPOLYGON GeoSeries (gpk_polygon_union): what a.polygon_union gives
    row-wise, over an explicit pair list.  Arguments, `drop_empty`, `return_status` and the returned tuple as polygon_clip_pairs."""
    mode = polygon_union_mode_arg(how, a._family(), b._family())
    return _polygon_pairs("gpk_polygon_union", mode, a, b, a_rows, b_rows, drop_empty, return_status)


def polygon_union_pairs_device(a: DeviceGeoArray, b: DeviceGeoArray, a_rows, b_rows, how: str = "union", drop_empty: bool = False, out_src=None,
                               out_status=None, stream: int = 0) -> GeoSeries:
    """Device-buffer variant, shaped like polygon_clip_pairs_device."""
    mode = polygon_union_mode_arg(how, a.geom_type, b.geom_type)
    n = a_rows.shape[0] if a_rows is not None else (b_rows.shape[0] if b_rows is not None else a.n_geoms)
    return polygon_clip_call(a, b, _ptr(a_rows), _ptr(b_rows), n, MEM_DEVICE, mode, _abi.CLIP_DROP_EMPTY if drop_empty else 0, _ptr(out_src), MEM_DEVICE,
                             _ptr(out_status), MEM_DEVICE, stream, entry="gpk_polygon_union")


# ---- polygon x polygon symmetric difference over a pair list (gpk_polygon_symdiff) -------------------------------------------------------

PSYMDIFF_MODES = {"symmetric_difference": _abi.PSYMDIFF_SYMMETRIC_DIFFERENCE}


def polygon_symdiff_mode_arg(how: str, a_family: int, b_family: int) -> int:
    """The GPK_PSYMDIFF_* mode of `how`, checked before any device call together with the families: polygons x polygons."""
    if how not in PSYMDIFF_MODES:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT,
                                     f"polygon symmetric difference: unknown how {how!r}: one of {sorted(PSYMDIFF_MODES)}")
    if a_family not in POLYGONAL or b_family not in POLYGONAL:
        raise _mismatch("polygon symmetric difference: Polygon | MultiPolygon x Polygon | MultiPolygon "
                        f"(found {_abi_name(a_family)} x {_abi_name(b_family)})")
    return PSYMDIFF_MODES[how]


def polygon_symdiff_pairs(a: GeoSeries, b: GeoSeries, left, right, drop_empty: bool = False, return_status: bool = False,
                          how: str = "symmetric_difference"):
    """symmetric_difference(a[left[k]], b[right[k]]) for every pair k, as a MULTIPOLYGON GeoSeries (gpk_polygon_symdiff): what
    a.polygon_symmetric_difference gives row-wise, over an explicit pair list.  Arguments, `drop_empty`, `return_status` and the
    returned tuple as polygon_clip_pairs."""
    mode = polygon_symdiff_mode_arg(how, a._family(), b._family())
    return _polygon_pairs("gpk_polygon_symdiff", mode, a, b, left, right, drop_empty, return_status)


def polygon_symdiff_pairs_device(a: DeviceGeoArray, b: DeviceGeoArray, left, right, drop_empty: bool = False, out_src=None, out_status=None,
                                 stream: int = 0, how: str = "symmetric_difference") -> GeoSeries:
    """Device-buffer variant, shaped like polygon_clip_pairs_device."""
    mode = polygon_symdiff_mode_arg(how, a.geom_type, b.geom_type)
    n = left.shape[0] if left is not None else (right.shape[0] if right is not None else a.n_geoms)
    return polygon_clip_call(a, b, _ptr(left), _ptr(right), n, MEM_DEVICE, mode, _abi.CLIP_DROP_EMPTY if drop_empty else 0, _ptr(out_src), MEM_DEVICE,
                             _ptr(out_status), MEM_DEVICE, stream, entry="gpk_polygon_symdiff")


@dataclass
class SpatialJoinOverlayArgs:
    """Options of spatial_join_overlay."""

    r_index: Optional[SpatialIndex] = None  # an index of `right` carrying the bbox grid


def spatial_join_overlay(left: GeoSeries, right: GeoSeries, how: str = "intersection", args: Optional[SpatialJoinOverlayArgs] = None):
    """GeoPandas' overlay(left, right, how=..., keep_geom_type=True) on two polygon layers as a pair list:
    gpk_polygon_relation_join(intersects), then gpk_polygon_clip over the returned pairs.  Returns (l, r, geometry): int64 row numbers
    of `left` and `right`, sorted by (l, r), and a MULTIPOLYGON GeoSeries.
      "intersection"  the pairs that share AREA, with that area — a pair that only touches is in the join and not here.
      "difference"    every pair of the join whose left row is not covered by its right row, with left[l] minus right[r]: ONE OUTPUT
                      ROW PER (l, r) PAIR, not GeoPandas' row-wise fold of a left row over all its partners (left rows without a
                      partner do not appear either).  The fold is out of scope."""
    args = args or SpatialJoinOverlayArgs()
    polygon_clip_mode_arg(how, left._family(), right._family())
    pairs, _counts, _masks = polygon_relation_pairs(left, right, "intersects", args.r_index)
    geometry, src = polygon_clip_pairs(left, right, pairs[:, 0], pairs[:, 1], how, drop_empty=True)
    kept = pairs[src]
    return kept[:, 0].astype(np.int64), kept[:, 1].astype(np.int64), geometry


# ---- line x line predicate join (gpk_line_relation_join) ---------------------------------------------------------------------

# GeoPandas' predicate names (plus `equals`) -> GPK_LL_PRED_*
LINE_RELATION_PREDICATES = {
    "intersects": _abi.LL_PRED_INTERSECTS,
    "within": _abi.LL_PRED_WITHIN,
    "contains": _abi.LL_PRED_CONTAINS,
    "covered_by": _abi.LL_PRED_COVERED_BY,
    "covers": _abi.LL_PRED_COVERS,
    "crosses": _abi.LL_PRED_CROSSES,
    "touches": _abi.LL_PRED_TOUCHES,
    "overlaps": _abi.LL_PRED_OVERLAPS,
    "equals": _abi.LL_PRED_EQUALS,
}


def line_relation_predicate_arg(predicate: str, left_family: int, right_family: int) -> int:
    """The GPK_LL_PRED_* id of a predicate name for a join of these two families, checked before any device call: a known name and
    both sides lineal.  The relation is always read "left row <predicate> right row"."""
    if predicate not in LINE_RELATION_PREDICATES:
        raise _abi.GeopolarsHipError(
            _abi.GPK_ERR_INVALID_ARGUMENT, f"line relation join: unknown predicate {predicate!r}: one of {sorted(LINE_RELATION_PREDICATES)}"
        )
    if left_family not in LINEAL or right_family not in LINEAL:
        raise _mismatch(
            f"line relation join: LineString | MultiLineString x LineString | MultiLineString (found {_abi_name(left_family)} x {_abi_name(right_family)})"
        )
    return LINE_RELATION_PREDICATES[predicate]


def line_relation_pairs(
    left: GeoSeries,
    right: GeoSeries,
    predicate: str = "intersects",
    r_index: Optional[SpatialIndex] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every (l, r) of two line columns (which may be the same column: junctions, duplicates) whose exact relation satisfies
    `predicate`: (pairs (H, 2) uint32 sorted by (l, r), counts (n_left,) uint32, masks (H,) uint8 — what
    left.line_relation(right) gives for the pairs).  Host-buffer variant: the pair buffer is sized like join_pairs'."""
    pred = line_relation_predicate_arg(predicate, left._family(), right._family())
    return _payload_pairs("gpk_line_relation_join", left, right, r_index, pred, left_row_base, payload=np.uint8)


def line_relation_pairs_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    predicate: str,
    out_counts,
    out_pairs,
    out_mask=None,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_mask (cap,) uint8 torch CUDA tensors (any may
    be None; out_pairs None = count only; without out_mask the work on a pair ends as soon as its predicate is settled) are filled in
    place on `stream`; returns the number of pairs."""
    pred = line_relation_predicate_arg(predicate, left.geom_type, right.geom_type)
    return _payload_pairs_device("gpk_line_relation_join", left, right, r_index, pred, out_counts, out_pairs, out_mask, left_row_base, stream)


def spatial_join_line_relation(lhs, rhs, options: Optional[SpatialJoinRelationArgs] = None):
    """GeoPandas' sjoin(predicate=...) over two pyarrow Tables of lines with a `geometry` column (WKB or native GeoArrow, as
    spatial_join takes them): every left row with every right row in the relation, shaped like spatial_join_relation's result —
    suffixed left columns, suffixed right columns, then `relation_col` (the pair's 7-bit mask) when asked for."""
    options = options or SpatialJoinRelationArgs()
    return _payload_table_join("line relation join", lhs, rhs, options, lambda: _known_predicate("line relation join", options.predicate, LINE_RELATION_PREDICATES), line_relation_pairs,
                               relation_col=options.relation_col)

# ---- point predicate join (gpk_point_relation_join) --------------------------------------------------------------------------------

# GeoPandas' predicate names (plus `equals`) -> GPK_PT_PRED_*
POINT_RELATION_PREDICATES = {
    "intersects": _abi.PT_PRED_INTERSECTS,
    "within": _abi.PT_PRED_WITHIN,
    "contains": _abi.PT_PRED_CONTAINS,
    "covered_by": _abi.PT_PRED_COVERED_BY,
    "covers": _abi.PT_PRED_COVERS,
    "crosses": _abi.PT_PRED_CROSSES,
    "touches": _abi.PT_PRED_TOUCHES,
    "overlaps": _abi.PT_PRED_OVERLAPS,
    "equals": _abi.PT_PRED_EQUALS,
}


def point_relation_predicate_arg(predicate: str, left_family: int, right_family: int) -> int:
    """The GPK_PT_PRED_* id of a predicate name for a join of these two families, checked before any device call and in the C ABI's
    order: a known name, then a POINT | MULTIPOINT column on at least one side.  The relation is always read "left row <predicate>
    right row"; the library transposes it when only the right side is punctual."""
    if predicate not in POINT_RELATION_PREDICATES:
        raise _abi.GeopolarsHipError(
            _abi.GPK_ERR_INVALID_ARGUMENT, f"point relation join: unknown predicate {predicate!r}: one of {sorted(POINT_RELATION_PREDICATES)}"
        )
    point_relation_sides("point relation join", left_family, right_family)
    return POINT_RELATION_PREDICATES[predicate]


def point_relation_pairs(
    left: GeoSeries,
    right: GeoSeries,
    predicate: str = "intersects",
    r_index: Optional[SpatialIndex] = None,
    left_row_base: int = 0,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every (l, r) of a point column and a column of any family, in either order (or one point column against itself: duplicates),
    with "left row <predicate> right row": (pairs (H, 2) uint32 sorted by (l, r), counts (n_left,) uint32, masks (H,) uint8 — the
    point relation mask of the pair, A = the punctual side, the left one when both are).  Host-buffer variant: the pair buffer is
    sized like join_pairs'."""
    pred = point_relation_predicate_arg(predicate, left._family(), right._family())
    return _payload_pairs("gpk_point_relation_join", left, right, r_index, pred, left_row_base, payload=np.uint8)


def point_relation_pairs_device(
    left: DeviceGeoArray,
    right: DeviceGeoArray,
    r_index: Optional[SpatialIndex],
    predicate: str,
    out_counts,
    out_pairs,
    out_mask=None,
    left_row_base: int = 0,
    stream: int = 0,
) -> int:
    """Device-buffer variant: out_counts (n,) uint32-as-int32, out_pairs (cap, 2) and out_mask (cap,) uint8 torch CUDA tensors (any may
    be None; out_pairs None = count only; without out_mask the work on a pair ends as soon as its predicate is settled) are filled in
    place on `stream`; returns the number of pairs."""
    pred = point_relation_predicate_arg(predicate, left.geom_type, right.geom_type)
    return _payload_pairs_device("gpk_point_relation_join", left, right, r_index, pred, out_counts, out_pairs, out_mask, left_row_base, stream)


def spatial_join_point_relation(lhs, rhs, options: Optional[SpatialJoinRelationArgs] = None):
    """GeoPandas' sjoin(predicate=...) over two pyarrow Tables with a `geometry` column (WKB or native GeoArrow, as spatial_join takes
    them), at least one of them of points: every left row with every right row in the relation, shaped like spatial_join_relation's
    result — suffixed left columns, suffixed right columns, then `relation_col` (the pair's 4-bit mask) when asked for."""
    options = options or SpatialJoinRelationArgs()
    return _payload_table_join("point relation join", lhs, rhs, options, lambda: _known_predicate("point relation join", options.predicate, POINT_RELATION_PREDICATES), point_relation_pairs,
                               relation_col=options.relation_col)


# ---- one join for every pair of families ---------------------------------------------------------------------------------------------

# predicate_route's relation family -> (the predicate names of its join, its pairs function)
SJOIN_ROUTES = {
    "point": (POINT_RELATION_PREDICATES, point_relation_pairs),
    "line": (LINE_RELATION_PREDICATES, line_relation_pairs),
    "polygon": (POLYGON_RELATION_PREDICATES, polygon_relation_pairs),
    "line_polygon": (RELATION_PREDICATES, relation_pairs),
}


def sjoin_pairs(left: GeoSeries, right: GeoSeries, predicate: str = "intersects", r_index: Optional[SpatialIndex] = None, left_row_base: int = 0):
    """(pairs, counts, masks) of "left row <predicate> right row" for any two families: the relation join that serves the pair
    (predicate_route) with its own predicate names and its own mask.  An unknown geometry type or a name the family does not have is
    refused before any device call."""
    route = predicate_route(left._family(), right._family())[0]
    names, pairs_fn = SJOIN_ROUTES[route]
    if predicate not in names:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"sjoin: unknown {route} join predicate {predicate!r}: one of {sorted(names)}")
    return pairs_fn(left, right, predicate, r_index, left_row_base)


def sjoin(lhs, rhs, predicate: str = "intersects", join_type: str = "inner", relation_col: Optional[str] = None, l_suffix: Optional[str] = "_left",
          r_suffix: Optional[str] = "_right", r_index: Optional[SpatialIndex] = None, l_geom_type: int = -1, r_geom_type: int = -1):
    """GeoPandas' sjoin(lhs, rhs, predicate=...) over two pyarrow Tables with a `geometry` column of any two families: the table join
    of the relation family that serves the pair (spatial_join_point_relation, _line_relation, _polygon_relation, _relation), chosen
    once the geometry columns are decoded.  `relation_col`: that family's mask of every pair."""
    options = SpatialJoinRelationArgs(predicate=predicate, join_type=join_type, relation_col=relation_col, l_suffix=l_suffix, r_suffix=r_suffix,
                                      r_index=r_index, l_geom_type=l_geom_type, r_geom_type=r_geom_type)
    every = set().union(*(names for names, _ in SJOIN_ROUTES.values()))
    return _payload_table_join("sjoin", lhs, rhs, options, lambda: _known_predicate("sjoin", predicate, {k: None for k in every}), sjoin_pairs,
                               relation_col=relation_col)
