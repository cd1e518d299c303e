"""`GeoSeries` — the host-side mirror of the reference's operator surface.

Same method names, argument meaning and error behaviour as `trait GeoSeries`
(geopolars/geopolars-geo/src/geoseries.rs:10-181) and its Python accessor `GeoRustSeries`
(py-geopolars/python/geopolars/internals/georust/geoseries.py:17-320), plus the north-star
predicates (`contains` / `within` / `intersects` / `bounds`) that exist in the reference only as
dead code (geopolars/src/spatial_index.rs:89-137).  polars is not available here, so a series is a
single-chunk GeoArrow array (`GeoArrowArray`) instead of a `polars.Series` — exactly what
ffi.rs:56 rechunks to before crossing into Rust.

Every operator — the structural ones (`geom_type`, `is_empty`, `x`, `y`, `exterior`, `explode`, `envelope`, `is_ring`)
included — goes through the C ABI into HIP kernels; nothing here computes geometry on the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Union

import numpy as np

from . import _abi
from ._abi import (
    GEOM_LINESTRING,
    GEOM_MULTILINESTRING,
    GEOM_MULTIPOINT,
    GEOM_MULTIPOLYGON,
    GEOM_POINT,
    GEOM_POLYGON,
    MEM_HOST,
    PREDICATES,
)
from .geoarrow import DeviceGeoArray, GeoArrowArray

TransformOrigin = Union[str, tuple]

SUPPORTED_CRS = "EPSG:4326 (OGC:CRS84), EPSG:3857, EPSG:3395, EPSG:32601-32660, EPSG:32701-32760"


def crs_supported(epsg: int) -> bool:
    """mirror of gpk_crs_supported (the argument checks need no library)"""
    return epsg in (4326, 3857, 3395) or 32601 <= epsg <= 32660 or 32701 <= epsg <= 32760


def parse_crs(crs) -> int:
    """ "EPSG:4326" in any letter case, "OGC:CRS84" or an int -> the EPSG code; ValueError for anything outside the analytic set"""
    code = None
    if isinstance(crs, (int, np.integer)) and not isinstance(crs, bool):
        code = int(crs)
    elif isinstance(crs, str):
        t = crs.strip().upper()
        if t == "OGC:CRS84":
            code = 4326
        elif t.startswith("EPSG:") and t[5:].isdigit():
            code = int(t[5:])
    if code is None or not crs_supported(code):
        raise ValueError(
            f"reproject: CRS {crs!r} is not in the analytic set ({SUPPORTED_CRS}); arbitrary CRS strings and datum shifts are "
            "the reference's PROJ path (to_crs, geoseries.rs:148-151)"
        )
    return code


def utm_crs_of_bounds(bounds) -> str:
    """estimate_utm_crs from an (n, 4) minx, miny, maxx, maxy array in lon/lat degrees (NaN rows — empty geometries — are ignored)"""
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 4)
    b = b[~np.isnan(b).any(axis=1)]
    if len(b) == 0:
        raise ValueError("estimate_utm_crs: the column has no coordinates")
    lon = 0.5 * (b[:, 0].min() + b[:, 2].max())
    lat = 0.5 * (b[:, 1].min() + b[:, 3].max())
    if not (-180.0 <= lon <= 180.0 and -90.0 <= lat <= 90.0):
        raise ValueError("estimate_utm_crs: the column is not in lon/lat degrees")
    zone = min(max(int(np.floor((lon + 180.0) / 6.0)) + 1, 1), 60)
    return f"EPSG:{(32600 if lat >= 0 else 32700) + zone}"


class GeoSeries:
    def __init__(self, array: Optional[GeoArrowArray], name: str = "geometry", device: Optional[DeviceGeoArray] = None):
        self._array = array
        self.name = name  # output column name is always "geometry" (util.rs:22,43,52)
        self._dev: Optional[DeviceGeoArray] = device

    @property
    def array(self) -> GeoArrowArray:
        """Host GeoArrow buffers; a series decoded on the GPU downloads them on first use."""
        if self._array is None:
            self._array = self._dev.download()
        return self._array

    # ---- construction --------------------------------------------------------------------------
    @staticmethod
    def from_wkb(column) -> "GeoSeries":
        return GeoSeries(GeoArrowArray.from_arrow_wkb(column))

    def to_wkb(self, on_device: bool = True) -> tuple[np.ndarray, np.ndarray]:
        """The series as a WKB column (values uint8, offsets int32) — the form geometry-valued results leave the
        reference in (from_geom_vec, util.rs:11-24).  Encoded on the GPU by default; on_device=False uses the host
        encoder (no device needed)."""
        if on_device:
            return self.device().to_wkb()
        return self.array.to_wkb()

    @staticmethod
    def from_wkb_device(values, offsets, validity=None) -> "GeoSeries":
        """WKB column decoded on the GPU: only the raw bytes are uploaded (gpk_geoarray_from_wkb)."""
        return GeoSeries(None, device=DeviceGeoArray.from_wkb(values, offsets, validity))

    @staticmethod
    def from_arrow(column, geom_type: int = -1) -> "GeoSeries":
        """`geopolars.from_arrow` (py-geopolars/src/ffi.rs:93-109 calls it on the way back; the Series it wraps crosses into Rust
        through the Arrow C Data Interface, :12-32): a pyarrow geometry column — WKB binary, or native GeoArrow with Struct<x, y>
        (internals/geoseries.py:86-113) or FixedSizeList<f64, 2> coordinates — handed to the library as the two exported structs
        (gpk_geoarray_from_arrow); the column lands in HBM without a host-side rewrite."""
        return GeoSeries(None, device=DeviceGeoArray.from_arrow(column, geom_type))

    @staticmethod
    def from_points(xy) -> "GeoSeries":
        return GeoSeries(GeoArrowArray.from_points(xy))

    def __len__(self) -> int:
        return self._dev.n_geoms if self._array is None else len(self._array)

    def device(self) -> DeviceGeoArray:
        """Upload on first use ("copied once to HBM"); later operators reuse the resident copy."""
        if self._dev is None:
            self._dev = DeviceGeoArray.upload(self.array)
        return self._dev

    @staticmethod
    def _rowwise(entry: str, a: "GeoSeries", b: "GeoSeries", rows: Optional[np.ndarray], out: np.ndarray, *mid) -> np.ndarray:
        """One row-wise call of the C ABI, entry(a, b, b_rows, *mid, out, MEM_HOST, stream), that fills `out` with one value per row; an
        empty column makes no call.  The callers have checked families and row pairing (the *_args functions below) before."""
        if len(out):
            _abi.check(getattr(_abi.lib(), entry)(a.device().handle, b.device().handle, None if rows is None else rows.ctypes.data, *mid,
                                                  out.ctypes.data, MEM_HOST, None))
        return out

    # ---- structural operators (gpk_structural.hip: maps over rows / offset surgery on the device) ---------------
    def _row_map(self, fn, dtype) -> np.ndarray:
        out = np.empty(len(self), dtype=dtype)
        _abi.check(fn(self.device().handle, out.ctypes.data if len(out) else None, MEM_HOST, None))
        return out

    def geom_type(self) -> np.ndarray:
        """geoseries.rs:60-73: -1 missing, 0 Point, 1 LineString, 3 Polygon, 4.., 6 MultiPolygon."""
        return self._row_map(_abi.lib().gpk_geom_type, np.int8)

    def is_empty(self) -> np.ndarray:
        """geoseries.rs:75-76 (geo HasDimensions::is_empty)."""
        return self._row_map(_abi.lib().gpk_is_empty, np.uint8).astype(bool)

    def x(self) -> np.ndarray:
        self._require(GEOM_POINT, "x")
        out = np.empty(len(self), dtype=np.float64)
        _abi.check(_abi.lib().gpk_point_xy(self.device().handle, out.ctypes.data, None, MEM_HOST, None))
        return out

    def y(self) -> np.ndarray:
        self._require(GEOM_POINT, "y")
        out = np.empty(len(self), dtype=np.float64)
        _abi.check(_abi.lib().gpk_point_xy(self.device().handle, None, out.ctypes.data, MEM_HOST, None))
        return out

    def exterior(self) -> "GeoSeries":
        """Outer ring of each polygon as a LineString series (geoseries.rs:43-47); null rows stay null."""
        self._require(GEOM_POLYGON, "exterior")
        a = self.array
        xy = np.empty((max(a.n_coords, 1), 2), dtype=np.float64)
        off = np.zeros(len(self) + 1, dtype=np.int32)
        n_out = C.c_int64(0)
        _abi.check(_abi.lib().gpk_exterior(self.device().handle, xy.ctypes.data, off.ctypes.data, C.byref(n_out), MEM_HOST, None))
        return GeoSeries(GeoArrowArray(GEOM_LINESTRING, xy[: int(n_out.value)].copy(), geom_offsets=off, validity=a.validity, n_geoms=len(self)))

    def is_ring(self) -> np.ndarray:
        """geoseries.rs:78-83: True for closed features (first coordinate == last; geo-types counts an empty linestring
        as closed); LineStrings only."""
        self._require(GEOM_LINESTRING, "is_ring")
        return self._row_map(_abi.lib().gpk_is_ring, np.uint8).astype(bool)

    def explode(self, return_parents: bool = False):
        """geoseries.rs:49-50: multi-part geometries -> one row per part.  Pure offset surgery on the device: the result
        views this series' coordinate buffer (benches/explode.rs explodes 45,000 two-point MultiPoints this way).  With
        `return_parents` also the row each member came from."""
        h = C.c_void_p()
        dev = self.device()
        sizes = (C.c_int64 * 4)()  # n_coords, n_parts, n_rings, n_geoms of the handle: no host copy of a series decoded on the GPU
        _abi.check(_abi.lib().gpk_geoarray_download(dev.handle, sizes, None, None, None, None, None))
        src_type = dev.geom_type
        n_members = {GEOM_MULTIPOINT: int(sizes[0]), GEOM_MULTILINESTRING: int(sizes[2]), GEOM_MULTIPOLYGON: int(sizes[1])}.get(src_type, len(self))
        parents = np.empty(n_members, dtype=np.int32) if return_parents else None
        _abi.check(_abi.lib().gpk_explode(dev.handle, parents.ctypes.data if return_parents and n_members else None, MEM_HOST, None, C.byref(h)))
        gt = {GEOM_MULTIPOINT: GEOM_POINT, GEOM_MULTILINESTRING: GEOM_LINESTRING, GEOM_MULTIPOLYGON: GEOM_POLYGON}.get(src_type, src_type)
        view = DeviceGeoArray(h.value, gt, n_members, int(sizes[0]), keepalive=[self._dev])  # the view borrows our buffers
        out = GeoSeries(None, device=view)
        return (out, parents) if return_parents else out

    def _require(self, t: int, op: str) -> None:
        if self.array.geom_type != t:
            raise _abi.MismatchedGeometry(
                _abi.GPK_ERR_MISMATCHED_GEOMETRY,
                f"{op}: expected {_abi_name(t)} (found {_abi_name(self.array.geom_type)})",
            )

    # ---- unary operators (HIP) -----------------------------------------------------------------
    def area(self) -> np.ndarray:
        out = np.empty(len(self), dtype=np.float64)
        _abi.check(_abi.lib().gpk_area(self.device().handle, out.ctypes.data, MEM_HOST, None))
        return out

    def signed_area(self) -> np.ndarray:
        out = np.empty(len(self), dtype=np.float64)
        _abi.check(_abi.lib().gpk_signed_area(self.device().handle, out.ctypes.data, MEM_HOST, None))
        return out

    def euclidean_length(self) -> np.ndarray:
        out = np.empty(len(self), dtype=np.float64)
        _abi.check(_abi.lib().gpk_euclidean_length(self.device().handle, out.ctypes.data, MEM_HOST, None))
        return out

    def bounds(self) -> np.ndarray:
        """(n, 4) minx, miny, maxx, maxy — the north-star `bounds`; NaN for empty geometries."""
        out = np.empty((len(self), 4), dtype=np.float64)
        _abi.check(_abi.lib().gpk_bounds(self.device().handle, out.ctypes.data, MEM_HOST, None))
        return out

    def envelope(self) -> "GeoSeries":
        """geoseries.rs:28-33: the bounding rectangle as a geometry.  Points stay points; everything
        else becomes the closed 5-coordinate rectangle polygon (minx miny, maxx miny, maxx maxy,
        minx maxy, minx miny) that geo's `Rect::to_polygon` produces; null and empty rows give null."""
        if self.array.geom_type == GEOM_POINT:
            return GeoSeries(self.array)
        n = len(self)
        xy = np.empty((5 * n, 2), dtype=np.float64)
        valid = np.empty(n, dtype=np.uint8)
        _abi.check(_abi.lib().gpk_envelope(self.device().handle, xy.ctypes.data if n else None, valid.ctypes.data if n else None, MEM_HOST, None))
        validity = None if valid.all() else np.packbits(valid.astype(bool), bitorder="little")
        return GeoSeries(
            GeoArrowArray(GEOM_POLYGON, xy, geom_offsets=np.arange(n + 1, dtype=np.int32), ring_offsets=np.arange(0, 5 * n + 1, 5, dtype=np.int32), validity=validity)
        )

    def centroid(self) -> "GeoSeries":
        xy = np.empty((len(self), 2), dtype=np.float64)
        valid = np.empty(len(self), dtype=np.uint8)
        _abi.check(_abi.lib().gpk_centroid(self.device().handle, xy.ctypes.data, valid.ctypes.data, MEM_HOST, None))
        ok = valid.astype(bool) & self.array.is_valid()  # null in, null out; an empty geometry has no centroid
        return GeoSeries(GeoArrowArray.from_points(xy, validity=None if ok.all() else np.packbits(ok, bitorder="little")))

    def representative_point(self, return_width: bool = False):
        """GeoPandas' representative_point (shapely point_on_surface, gpk_representative_point): a POINT series with one point per row
        that lies in the row's geometry — the midpoint of the widest section of a scan line through a polygon, the interior vertex of
        a line nearest to its centroid, the member of a multipoint nearest to the mean — where `centroid` often falls outside.  Null
        where there is none (a null or empty row, a non-finite coordinate).  With `return_width` also the float64 width of the chosen
        section (0: a degenerate polygon answered its first coordinate; NaN for lines, points and null rows)."""
        return_width = return_width_arg(return_width)
        n = len(self)
        xy = np.empty((n, 2), dtype=np.float64)
        valid = np.empty(n, dtype=np.uint8)
        width = np.empty(n, dtype=np.float64) if return_width else None
        if n:
            _abi.check(_abi.lib().gpk_representative_point(
                self.device().handle, xy.ctypes.data, valid.ctypes.data, width.ctypes.data if return_width else None, MEM_HOST, None))
        ok = valid.astype(bool)
        pts = GeoSeries(GeoArrowArray.from_points(xy, validity=None if ok.all() else np.packbits(ok, bitorder="little")))
        return (pts, width) if return_width else pts

    def point_on_surface(self, return_width: bool = False):
        """shapely's name of representative_point"""
        return self.representative_point(return_width)

    def convex_hull(self) -> "GeoSeries":
        a = self.array
        xy = np.empty((a.n_coords + len(self), 2), dtype=np.float64)
        ring_off = np.empty(len(self) + 1, dtype=np.int32)
        _abi.check(_abi.lib().gpk_convex_hull(self.device().handle, xy.ctypes.data, ring_off.ctypes.data, MEM_HOST, None))
        xy = xy[: ring_off[-1]]
        return GeoSeries(
            GeoArrowArray(GEOM_POLYGON, xy, geom_offsets=np.arange(len(self) + 1, dtype=np.int32), ring_offsets=ring_off, validity=a.validity)
        )

    def minimum_rotated_rectangle(self) -> "GeoSeries":
        """GeoPandas' minimum_rotated_rectangle (shapely oriented_envelope, gpk_minimum_rotated_rectangle): a POLYGON series with the
        least-area rectangle on an edge of the row's convex hull as one closed 5-coordinate ring per row (a single point: the point five
        times; collinear coordinates p .. q: p q q p p).  A row without an answer (no coordinate, a non-finite coordinate) becomes an
        empty polygon; a null row stays null."""
        n = len(self)
        xy = np.empty((5 * n, 2), dtype=np.float64)
        valid = np.empty(n, dtype=np.uint8)
        if n:
            _abi.check(_abi.lib().gpk_minimum_rotated_rectangle(self.device().handle, xy.ctypes.data, valid.ctypes.data, MEM_HOST, None))
        return _ring_series(xy, valid.astype(bool), 5, self.array.validity)

    def oriented_envelope(self) -> "GeoSeries":
        """shapely's name of minimum_rotated_rectangle"""
        return self.minimum_rotated_rectangle()

    def _bounding_circle(self, want_centre: bool):
        n = len(self)
        centre = np.empty((n, 2), dtype=np.float64) if want_centre else None
        radius = np.empty(n, dtype=np.float64)
        valid = np.empty(n, dtype=np.uint8)
        if n:
            _abi.check(_abi.lib().gpk_minimum_bounding_circle(
                self.device().handle, centre.ctypes.data if want_centre else None, radius.ctypes.data, valid.ctypes.data, MEM_HOST, None))
        return centre, radius, valid.astype(bool)

    def minimum_bounding_radius(self) -> np.ndarray:
        """GeoPandas' minimum_bounding_radius (gpk_minimum_bounding_circle): the float64 radius of the smallest circle that contains the
        row's coordinates; NaN where there is none (a null or empty row, a non-finite coordinate)."""
        return self._bounding_circle(False)[1]

    def minimum_bounding_circle_parts(self):
        """(POINT series of the centres, float64 radii) of the smallest circle that contains each row's coordinates; a row without an
        answer is a null point and a NaN radius."""
        centre, radius, ok = self._bounding_circle(True)
        return GeoSeries(GeoArrowArray.from_points(centre, validity=None if ok.all() else np.packbits(ok, bitorder="little"))), radius

    def minimum_bounding_circle(self, quad_segs: int = 8) -> "GeoSeries":
        """GeoPandas' minimum_bounding_circle: a POLYGON series, the smallest circle that contains each row's coordinates as a ring of
        4 * quad_segs + 1 coordinates centre + r (cos t, sin t), counter-clockwise from t = 0, the last coordinate the first bit for
        bit.  Centre and radius come from the GPU (gpk_minimum_bounding_circle); the ring is laid out here.  A radius-0 row gives the
        point repeated; a row without an answer an empty polygon; a null row stays null."""
        quad_segs = quad_segs_arg(quad_segs)
        centre, radius, ok = self._bounding_circle(True)
        return _ring_series(circle_rings(centre, radius, quad_segs), ok, 4 * quad_segs + 1, self.array.validity)

    def affine_transform(self, matrix: Sequence[float]) -> "GeoSeries":
        """matrix = [a, b, xoff, d, e, yoff] — the order `AffineTransform::from([f64; 6])` takes and
        py-geopolars/src/geo.rs:10-16 forwards (NOT the [a,b,d,e,xoff,yoff] of the Python docstring,
        georust/geoseries.py:33)."""
        m = (C.c_double * 6)(*[float(v) for v in matrix])
        a = self.array
        out = np.empty_like(a.xy)
        _abi.check(_abi.lib().gpk_affine_transform(self.device().handle, m, out.ctypes.data, MEM_HOST, None))
        return GeoSeries(
            GeoArrowArray(a.geom_type, out, a.geom_offsets, a.part_offsets, a.ring_offsets, a.validity, n_geoms=a.n_geoms)
        )

    def translate(self, xoff: float = 0.0, yoff: float = 0.0) -> "GeoSeries":
        """geoseries.rs:163-174; parameter names of the Python surface (georust/geoseries.py:278)"""
        return self.affine_transform([1.0, 0.0, xoff, 0.0, 1.0, yoff])

    GEODESIC_METHODS = {"geodesic": 0, "haversine": 1, "vincenty": 2}

    def geodesic_length(self, method: str = "geodesic") -> np.ndarray:
        """geoseries.rs:52-58 / georust/geoseries.py: metres, coordinates in (lon, lat) degrees; all three methods run on the
        GPU — 'geodesic' (the default) is Karney's algorithm, as in geo's GeodesicLength: the inverse of csrc/gpk_geodesic.h, which
        geodesic_distance runs too (the same bits); that header also holds the haversine and Vincenty formulas."""
        m = self.GEODESIC_METHODS.get(method.lower())
        if m is None:
            raise ValueError("Geodesic calculation method not valid. Use one of geodesic, haversine or vincenty")  # geo.rs:68-71
        out = np.empty(len(self), dtype=np.float64)
        _abi.check(_abi.lib().gpk_geodesic_length(self.device().handle, m, out.ctypes.data if len(out) else None, MEM_HOST, None))
        return out

    # ---- geodesic measures on WGS84 (gpk_geodesic.hip; geo's GeodesicArea / Distance / Bearing / Destination) -------------------------
    def _geodesic_area(self, flags: int, want_area: bool) -> np.ndarray:
        out = np.empty(len(self), dtype=np.float64)
        if len(out):
            ptr = out.ctypes.data
            _abi.check(_abi.lib().gpk_geodesic_area(self.device().handle, flags, ptr if want_area else None, None if want_area else ptr, MEM_HOST, None))
        return out

    def geodesic_area(self, signed: bool = False) -> np.ndarray:
        """Area in m^2 on the WGS84 ellipsoid of (lon, lat) polygons whose edges are shortest geodesics (Karney's order-6 series).
        signed=False: sum over parts of |shell| - sum |hole| (a ring covering more than half the ellipsoid reports its complement);
        signed=True: the sum of every ring's signed area as stored, counter-clockwise positive, each in (-A0/2, A0/2].  Rings around a
        pole or across the antimeridian are handled.  Non-polygonal rows: 0; null rows and rows with a latitude outside [-90, 90]: NaN."""
        return self._geodesic_area(_abi.GEODESIC_AREA_SIGNED if bool_arg("geodesic_area", "signed", signed) else 0, True)

    def geodesic_perimeter(self) -> np.ndarray:
        """Metres around EVERY ring of every part of a (lon, lat) polygon column, holes included (geodesic_length counts exterior rings
        only).  Non-polygonal rows: 0; null rows: NaN."""
        return self._geodesic_area(0, False)

    def _geodesic_inverse(self, op: str, other: "GeoSeries", other_rows, which: int) -> np.ndarray:
        geodesic_points_arg(op, self, other)
        rows = distance_rows_arg(op, self, other, other_rows)
        out = np.empty(len(self), dtype=np.float64)
        if len(out):
            ptrs = [None, None, None]
            ptrs[which] = out.ctypes.data
            _abi.check(_abi.lib().gpk_geodesic_inverse(self.device().handle, other.device().handle, None if rows is None else rows.ctypes.data, *ptrs,
                                                       MEM_HOST, None))
        return out

    def geodesic_distance(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """Metres along the WGS84 ellipsoid between the POINT rows of self and other (row i with other[other_rows[i]] when given);
        coordinates are (lon, lat) degrees.  NaN for a null or empty row, a NaN coordinate or a latitude outside [-90, 90]."""
        return self._geodesic_inverse("geodesic_distance", other, other_rows, 0)

    def geodesic_bearing(self, other: "GeoSeries", final: bool = False, other_rows=None) -> np.ndarray:
        """Forward azimuth in degrees clockwise from north, in [-180, 180], of the geodesic from each POINT of self to the POINT of
        other: at the start (final=False) or on arrival (final=True)."""
        return self._geodesic_inverse("geodesic_bearing", other, other_rows, 2 if bool_arg("geodesic_bearing", "final", final) else 1)

    def geodesic_destination(self, bearing, distance) -> "GeoSeries":
        """The POINT column reached from every POINT row along `bearing` (degrees clockwise from north) for `distance` metres on the
        WGS84 ellipsoid; each is a scalar or one value per row.  Longitudes come back in [-180, 180]; null rows stay null."""
        geodesic_points_arg("geodesic_destination", self, self)
        azi, s12 = (geodesic_values_arg("geodesic_destination", name, v, len(self)) for name, v in (("bearing", bearing), ("distance", distance)))
        out = np.empty((len(self), 2), dtype=np.float64)
        if len(out):
            _abi.check(_abi.lib().gpk_geodesic_direct(self.device().handle, azi.ctypes.data, len(azi), s12.ctypes.data, len(s12), out.ctypes.data, None,
                                                      MEM_HOST, None))
        return GeoSeries(GeoArrowArray(GEOM_POINT, out, validity=self.array.validity, n_geoms=len(self)))

    def simplify(self, tolerance: float) -> "GeoSeries":
        """geoseries.rs:108-116: Douglas-Peucker with geo 0.27's rules (gpk_simplify); the nesting above the coordinate
        sequences is unchanged."""
        a = self.array
        if a.geom_type in (GEOM_POINT, GEOM_MULTIPOINT):
            return GeoSeries(a)
        n_seq = a.n_rings if a.ring_offsets is not None else len(self)
        xy = np.empty((max(a.n_coords, 1), 2), dtype=np.float64)
        off = np.zeros(n_seq + 1, dtype=np.int32)
        n_out = C.c_int64(0)
        _abi.check(_abi.lib().gpk_simplify(self.device().handle, float(tolerance), xy.ctypes.data, off.ctypes.data, C.byref(n_out), MEM_HOST, None))
        xy = xy[: int(n_out.value)].copy()
        if a.ring_offsets is not None:
            return GeoSeries(GeoArrowArray(a.geom_type, xy, a.geom_offsets, a.part_offsets, off, a.validity, n_geoms=a.n_geoms))
        return GeoSeries(GeoArrowArray(a.geom_type, xy, off, validity=a.validity, n_geoms=a.n_geoms))

    # ---- analytic reprojection (gpk_crs.hip) ----------------------------------------------------------------------------------------
    def reproject(self, from_crs, to_crs, errors: str = "raise") -> "GeoSeries":
        """Reproject every coordinate between the analytic systems on the WGS84 ellipsoid: EPSG:4326 (x = lon, y = lat; also
        "OGC:CRS84"), 3857, 3395 and the UTM zones 32601-32660 / 32701-32760.  A CRS is "EPSG:nnnn" in any letter case,
        "OGC:CRS84" or an int.  One kernel launch (gpk_reproject); offsets and validity are carried over unchanged.

        A coordinate fails when it is non-finite, a geographic latitude is beyond +-90, a UTM destination is 90 degrees or
        more from its central meridian, or the result is non-finite (a Mercator at a pole).  errors="raise": ValueError with
        the count (the reference fails the whole call on one ProjError); errors="nan": failed coordinates come back NaN."""
        if errors not in ("raise", "nan"):
            raise ValueError('errors must be "raise" or "nan"')
        src, dst = parse_crs(from_crs), parse_crs(to_crs)
        a = self.array
        out = np.empty_like(a.xy)
        n_failed = C.c_int64(0)
        _abi.check(_abi.lib().gpk_reproject(self.device().handle, src, dst, out.ctypes.data if len(out) else None, C.byref(n_failed), MEM_HOST, None))
        if n_failed.value and errors == "raise":
            raise ValueError(f"reproject EPSG:{src} -> EPSG:{dst}: {n_failed.value} of {len(out)} coordinates failed (errors='nan' returns them as NaN)")
        return GeoSeries(GeoArrowArray(a.geom_type, out, a.geom_offsets, a.part_offsets, a.ring_offsets, a.validity, n_geoms=a.n_geoms))

    def estimate_utm_crs(self) -> str:
        """GeoPandas' name: the UTM zone of the centre of the column's total bounds (lon/lat degrees), as "EPSG:326zz" (centre
        latitude >= 0) or "EPSG:327zz".  zone = clamp(floor((lon + 180) / 6) + 1, 1, 60); the Norway and Svalbard exceptions
        of the UTM grid are NOT applied.  The bounds come from the `bounds` kernel."""
        return utm_crs_of_bounds(self.bounds())

    # ---- the one operator of the reference surface that stays off this backend ---------------------
    def to_crs(self, from_crs: str, to_crs: str) -> "GeoSeries":
        """The general PROJ entry (arbitrary CRS strings, datum shifts, grids) stays with the reference; the analytic same-datum
        systems — WGS84 lon/lat, both Mercators, UTM — are `reproject`."""
        raise NotImplementedError("to_crs (geoseries.rs:148-151, PROJ) is not on the accelerated path: use the reference's CPU implementation")

    def _about_origin(self, kind: int, p0: float, p1: float, origin: TransformOrigin) -> "GeoSeries":
        """rotate / scale / skew: the per-geometry origins (TransformOrigin, py-geopolars/src/utils.rs:5-27: 'centroid' |
        'center' of the bbox | (x, y)) and matrices are computed on the device (gpk_affine_about_origin)."""
        ox = oy = 0.0
        if isinstance(origin, str):
            o = origin.lower()
            if o not in ("centroid", "center"):
                raise ValueError("Invalid argument")  # PyGeopolarsError::Other("Invalid argument"), utils.rs:21
            ok = 0 if o == "centroid" else 1
        else:
            ok = 2
            ox, oy = (float(v) for v in origin)
        a = self.array
        out = np.empty_like(a.xy)
        _abi.check(_abi.lib().gpk_affine_about_origin(self.device().handle, kind, float(p0), float(p1), ok, ox, oy, out.ctypes.data if len(out) else None, MEM_HOST, None))
        return GeoSeries(GeoArrowArray(a.geom_type, out, a.geom_offsets, a.part_offsets, a.ring_offsets, a.validity, n_geoms=a.n_geoms))

    def rotate(self, angle: float, origin: TransformOrigin = "center") -> "GeoSeries":
        """angle in degrees, counter-clockwise, about `origin` (geoseries.rs:85-93)."""
        return self._about_origin(0, angle, 0.0, origin)

    def scale(self, xfact: float = 1.0, yfact: float = 1.0, origin: TransformOrigin = "center") -> "GeoSeries":
        return self._about_origin(1, xfact, yfact, origin)

    def skew(self, xs: float = 0.0, ys: float = 0.0, origin: TransformOrigin = "center") -> "GeoSeries":
        """geoseries.rs:118-139: [[1, tan(xs), xoff], [tan(ys), 1, yoff]], xoff = -origin.y*tan(xs),
        yoff = -origin.x*tan(ys); angles in degrees."""
        return self._about_origin(2, xs, ys, origin)

    # ---- binary row-wise operators (HIP) ---------------------------------------------------------
    def distance(self, other: "GeoSeries", other_rows: Optional[np.ndarray] = None, row_map: Optional["RowMap"] = None) -> np.ndarray:
        """geoseries.rs:141-146: 1-to-1 row-wise Euclidean distance.  `other_rows` pairs row i with
        other[other_rows[i]] (the take() a dataframe caller would have materialised); a `row_map` prepared once from
        such a pairing (RowMap(other, other_rows)) skips the per-call ordering of the rows.

        Every pair of families runs on the GPU.  When neither side is a POINT column: NaN for a null or empty row, 0.0
        exactly when the two geometries intersect (exact orientations), else the set distance (include/geopolars_hip.h,
        gpk_distance_rowwise).  The result has one value per row of `self` (with `other_rows`, or when `self` is a POINT
        column or neither side is), else per row of `other`: the two then have equally many rows."""
        if row_map is not None:
            out = np.empty(len(self), dtype=np.float64)
            _abi.check(_abi.lib().gpk_distance_rowmap(self.device().handle, other.device().handle, row_map.handle, out.ctypes.data, MEM_HOST, None))
            return out
        n = len(self) if self.array.geom_type == GEOM_POINT or other_rows is not None else len(other)
        out = np.empty(n, dtype=np.float64)
        rows = None if other_rows is None else row_map_arg("distance", other_rows, len(self))
        _abi.check(
            _abi.lib().gpk_distance_rowwise(
                self.device().handle, other.device().handle, None if rows is None else rows.ctypes.data, out.ctypes.data, MEM_HOST, None
            )
        )
        return out

    def hausdorff_distance(self, other: "GeoSeries", densify=None, other_rows=None) -> np.ndarray:
        """GeoPandas' GeoSeries.hausdorff_distance: the discrete Hausdorff distance of row i and other[other_rows[i]], between the
        rows' boundaries (gpk_hausdorff_distance; every pair of families).  `densify` is GeoPandas' fraction in (0, 1]: every segment
        is cut into k = round(1 / densify) equal parts whose ends are samples; None means the vertices alone.  NaN for a null or empty
        row; identical rows give exactly 0.0; hausdorff_distance(a, b) and (b, a) are the same doubles."""
        k = densify_arg("hausdorff_distance", densify)
        rows = distance_rows_arg("hausdorff_distance", self, other, other_rows)
        return self._rowwise("gpk_hausdorff_distance", self, other, rows, np.empty(len(self), dtype=np.float64), k)

    def frechet_distance(self, other: "GeoSeries", densify=None, other_rows=None, errors: str = "raise") -> np.ndarray:
        """GeoPandas' GeoSeries.frechet_distance: the discrete Frechet distance of row i and other[other_rows[i]] over the samples that
        `densify` defines (see hausdorff_distance), LINESTRING columns only (gpk_frechet_distance).  NaN for a null or empty row.  A
        row whose shorter side has more than GPK_FRECHET_MAX_SHORT samples is not computed: errors="raise" makes that a ValueError
        naming the count and the cap, errors="nan" returns NaN for such rows."""
        if errors not in ("raise", "nan"):
            raise ValueError('errors must be "raise" or "nan"')
        k = densify_arg("frechet_distance", densify)
        for side in (self, other):
            if side._family() != GEOM_LINESTRING:
                raise _mismatch(f"frechet_distance: LineString x LineString only, the measure is defined on one ordered sequence per side (found {_abi_name(side._family())})")
        rows = distance_rows_arg("frechet_distance", self, other, other_rows)
        out = np.empty(len(self), dtype=np.float64)
        if len(out) == 0:
            return out
        n_over = C.c_int64(0)
        _abi.check(
            _abi.lib().gpk_frechet_distance(
                self.device().handle, other.device().handle, None if rows is None else rows.ctypes.data, k, out.ctypes.data, C.byref(n_over), MEM_HOST, None
            )
        )
        if n_over.value and errors == "raise":
            raise ValueError(
                f"frechet_distance: {n_over.value} of {len(out)} rows have more than {FRECHET_MAX_SHORT} samples on their shorter side "
                "(errors='nan' returns them as NaN)"
            )
        return out

    def _predicate(self, other: "GeoSeries", name: str, other_rows=None) -> np.ndarray:
        out = np.empty(len(self), dtype=np.uint8)
        rows = None if other_rows is None else row_map_arg(name, other_rows, len(self))
        _abi.check(
            _abi.lib().gpk_predicate_rowwise(
                self.device().handle, other.device().handle, None if rows is None else rows.ctypes.data, PREDICATES[name], out.ctypes.data, MEM_HOST, None
            )
        )
        return out.astype(bool)

    def contains(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        return self._predicate(other, "contains", other_rows)

    def within(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        return self._predicate(other, "within", other_rows)

    def intersects(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        return self._predicate(other, "intersects", other_rows)

    def dwithin(self, other: "GeoSeries", distance: float, other_rows=None) -> np.ndarray:
        """GeoPandas' GeoSeries.dwithin: row i is True when distance(self[i], other[other_rows[i]]) <= `distance` (closed; the
        distance is the one `distance()` returns for the pair).  Null, empty and NaN-point rows are never within any distance.
        Every pair of families (gpk_dwithin_rowwise); `distance` must be finite and >= 0."""
        d = dwithin_distance_arg(distance)
        out = np.empty(len(self), dtype=np.uint8)
        rows = None if other_rows is None else row_map_arg("dwithin", other_rows, len(self))
        _abi.check(
            _abi.lib().gpk_dwithin_rowwise(
                self.device().handle, other.device().handle, None if rows is None else rows.ctypes.data, d, out.ctypes.data, MEM_HOST, None
            )
        )
        return out.astype(bool)

    # ---- line x polygon relations (gpk_linearea.hip) ---------------------------------------------
    def line_polygon_relation(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """The exact relation mask (uint8) of every row's line against its polygon (gpk_line_polygon_relation): bit 1 — the line has a
        point in the polygon's interior, 2 — on one of its rings, 4 — outside it or strictly inside a hole; 0 for a null or empty row,
        a NaN coordinate or an invalid ring.  One side is a LINESTRING / MULTILINESTRING column and the other a POLYGON / MULTIPOLYGON
        column, in either order; `other_rows` pairs row i with other[other_rows[i]] and needs `self` to be the lineal side."""
        line_first = relation_sides("line_polygon_relation", self._family(), other._family())
        rows = relation_rows_arg("line_polygon_relation", self, other, other_rows, line_first)
        lines, polys = (self, other) if line_first else (other, self)
        return self._rowwise("gpk_line_polygon_relation", lines, polys, rows, np.empty(len(lines), dtype=np.uint8))

    def _relation(self, other: "GeoSeries", name: str, other_rows=None) -> np.ndarray:
        a, b = self._family(), other._family()
        if a in POLYGONAL and b in POLYGONAL:
            return polygon_mask_predicate(self.polygon_relation(other, other_rows), name)
        if not ((a in LINEAL and b in POLYGONAL) or (a in POLYGONAL and b in LINEAL)):
            raise NotImplementedError(f"{name}: defined for LineString | MultiLineString x Polygon | MultiPolygon, not for {_abi_name(a)} x {_abi_name(b)}")
        mask = self.line_polygon_relation(other, other_rows)
        # the asymmetric names say which side is covered: a line covers no polygon, and no polygon is covered by a line
        if name in ("covered_by", "covers") and (a in LINEAL) != (name == "covered_by"):
            return np.zeros(len(mask), dtype=bool)
        return mask_predicate(mask, name)

    def crosses(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """the line has a point in the polygon's interior and one in its exterior (either order of the two families)"""
        return self._relation(other, "crosses", other_rows)

    def touches(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """the line meets the polygon's boundary but not its interior (either order of the two families)"""
        return self._relation(other, "touches", other_rows)

    def covered_by(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """no point of the line `self[i]` lies outside the polygon `other[i]`; always False with the polygons in `self`"""
        return self._relation(other, "covered_by", other_rows)

    def covers(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """no point of the line `other[i]` lies outside the polygon `self[i]`; always False with the lines in `self`"""
        return self._relation(other, "covers", other_rows)

    def disjoint(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """the line and the polygon share no point (False, like every relation, for unusable rows)"""
        return self._relation(other, "disjoint", other_rows)

    # ---- polygon x polygon relations (gpk_polyrel.hip) -------------------------------------------
    def polygon_relation(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """The exact relation mask (uint8) of every row's polygon A against its polygon B = other[other_rows[i]]
        (gpk_polygon_relation): bit 1 — the interiors share a point, 2 — a ring of A and a ring of B share a point, 4 — A's interior has
        a point outside B, 8 — B's interior has a point outside A; 0 for a null or empty row or an invalid ring on either side.  Both
        columns are POLYGON / MULTIPOLYGON.  crosses, touches, covers, covered_by and disjoint take two such columns too."""
        rows = polygon_relation_args("polygon_relation", self, other, other_rows)
        return self._rowwise("gpk_polygon_relation", self, other, rows, np.empty(len(self), dtype=np.uint8))

    def _polygon_relation(self, other: "GeoSeries", name: str, other_rows=None) -> np.ndarray:
        a, b = self._family(), other._family()
        if not (a in POLYGONAL and b in POLYGONAL):
            raise NotImplementedError(f"{name}: defined for Polygon | MultiPolygon x Polygon | MultiPolygon, not for {_abi_name(a)} x {_abi_name(b)}")
        return polygon_mask_predicate(self.polygon_relation(other, other_rows), name)

    def overlaps(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """the two polygons share area and each has area outside the other"""
        return self._polygon_relation(other, "overlaps", other_rows)

    def geom_equals(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """the two polygons are the same point set, however their rings are written (start, winding, extra collinear vertices, order
        of the parts)"""
        return self._polygon_relation(other, "equals", other_rows)

    def contains_properly(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """the polygon `other[i]` lies in the interior of `self[i]`: contained without touching its boundary"""
        return self._polygon_relation(other, "contains_properly", other_rows)

    # ---- intersection area and length (gpk_overlay.hip) ------------------------------------------
    def _intersection_measure(self, op: str, first, other: "GeoSeries", other_rows) -> np.ndarray:
        rows = intersection_measure_args(op, first, self, other, other_rows)
        return self._rowwise("gpk_intersection_measure", self, other, rows, np.empty(len(self), dtype=np.float64))

    def intersection_area(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """The area (float64) every row's polygon shares with its polygon other[other_rows[i]] (gpk_intersection_measure), without
        building the intersection: within 1e-9 * (d_a^2 + d_b^2) of the exact area for valid rows, d = the diagonal of a row's box.
        NaN for a null or empty row or an invalid ring on either side.  Both columns are POLYGON / MULTIPOLYGON."""
        return self._intersection_measure("intersection_area", POLYGONAL, other, other_rows)

    def intersection_length(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """The length (float64) of every row's line inside its closed polygon other[other_rows[i]] (gpk_intersection_measure): pieces
        along a ring count, a stretch the line runs over twice counts twice; within 1e-9 * length(line) of the exact length.  NaN for a
        null or empty row, a NaN or infinite line coordinate or an invalid ring.  self is LINESTRING / MULTILINESTRING, other POLYGON /
        MULTIPOLYGON."""
        return self._intersection_measure("intersection_length", LINEAL, other, other_rows)

    # ---- clip lines to polygons (gpk_lineclip.hip) ------------------------------------------------
    def _line_clip(self, op: str, mode: int, other: "GeoSeries", other_rows) -> "GeoSeries":
        rows = line_clip_args(op, self, other, other_rows)
        return line_clip_call(self.device(), other.device(), None, None if rows is None else rows.ctypes.data, len(self), MEM_HOST, mode, 0, None, MEM_HOST)

    def intersection(self, other: "GeoSeries", other_rows=None) -> "GeoSeries":
        """The piece of every row's line inside its closed polygon other[other_rows[i]] (gpk_line_clip), as a MULTILINESTRING series:
        one part per maximal run of the line in the polygon's interior or along a ring, in the order the line is walked; a valid row
        without parts where the two share no piece of positive length; a null row where intersection_length gives NaN.  Coordinates
        are the line's or the polygon's own, bit for bit, or crossings within 1e-9 of the pair's box diagonal of both carriers.
        self is LINESTRING / MULTILINESTRING, other POLYGON / MULTIPOLYGON."""
        return self._line_clip("intersection", _abi.CLIP_INSIDE, other, other_rows)

    def difference(self, other: "GeoSeries", other_rows=None) -> "GeoSeries":
        """The piece of every row's line outside its polygon other[other_rows[i]] — outside every part or inside a hole — closed
        (gpk_line_clip); shaped and ruled like `intersection`."""
        return self._line_clip("difference", _abi.CLIP_OUTSIDE, other, other_rows)

    # ---- polygon x polygon intersection and difference (gpk_polyclip.hip) --------------------------
    def _polygon_clip(self, op: str, mode: int, other: "GeoSeries", other_rows, return_status: bool, entry: str = "gpk_polygon_clip"):
        rows = polygon_clip_args(op, self, other, other_rows)
        status = np.empty(len(self), dtype=np.uint8) if return_status else None
        out = polygon_clip_call(self.device(), other.device(), None, None if rows is None else rows.ctypes.data, len(self), MEM_HOST, mode, 0, None,
                                MEM_HOST, None if status is None else status.ctypes.data, MEM_HOST, entry=entry)
        return (out, status) if return_status else out

    def polygon_intersection(self, other: "GeoSeries", other_rows=None, return_status: bool = False):
        """The area every row's polygon shares with other[other_rows[i]] (gpk_polygon_clip), as a MULTIPOLYGON series: the regularised
        intersection, the closure of int(a) ∩ int(b) — points and edges the two merely share leave no trace (GeoPandas'
        keep_geom_type=True).  A valid row without parts where the two share no area; a null row where intersection_area gives NaN.
        Coordinates are those of either operand, bit for bit, or crossings within 1e-9 of the pair's box diagonal of both carrying
        edges.  With `return_status` the result is (series, status): uint8 per row, 0 OK, 1 OK with a ring that touches itself at a
        point, 2 empty, 3 null input, 4 unresolved (a null row; only for invalid polygons or transitions closer than 1e-6 of their
        segment).  Both columns are POLYGON / MULTIPOLYGON."""
        return self._polygon_clip("polygon_intersection", _abi.PCLIP_INTERSECTION, other, other_rows, return_status)

    def polygon_difference(self, other: "GeoSeries", other_rows=None, return_status: bool = False):
        """The area of every row's polygon outside other[other_rows[i]], closed (gpk_polygon_clip): the regularised difference, the
        closure of int(a) minus b; a valid row without parts where b covers a.  Shaped and ruled like `polygon_intersection`."""
        return self._polygon_clip("polygon_difference", _abi.PCLIP_DIFFERENCE, other, other_rows, return_status)

    # ---- rows of the column (gpk_geotake.hip) ------------------------------------------------------------
    def take(self, idx, allow_null: bool = False) -> "GeoSeries":
        """Rows `idx` — any order, repeats allowed — as a device-resident series of the same type (gpk_geoarray_take): every level
        and the coordinates copied bit for bit on the device.  With `allow_null` an index of -1 gives a null row (a left join's
        unmatched side); without it every index must lie in [0, len)."""
        idx = take_args("take", self, idx, allow_null)
        return GeoSeries(None, name=self.name, device=self.device().take(idx))

    def filter(self, mask) -> "GeoSeries":
        """The rows a bool mask keeps, in order, as a device-resident series (gpk_geoarray_filter)."""
        mask = filter_args("filter", self, mask)
        return GeoSeries(None, name=self.name, device=self.device().filter(mask))

    def __getitem__(self, key) -> "GeoSeries":
        """s[a:b:c] (take of the range), s[bool array] (filter), s[integer array] (take).  One row is not a series: a scalar is
        refused."""
        if isinstance(key, slice):
            return self.take(np.arange(*key.indices(len(self)), dtype=np.int64))
        k = np.asarray(key)
        if k.ndim == 0:
            raise _abi.GeopolarsHipError(
                _abi.GPK_ERR_INVALID_ARGUMENT, f"GeoSeries[{key!r}]: one row is not a series: index with a slice, a bool mask or an integer array")
        return self.filter(k) if k.dtype == np.bool_ else self.take(k)

    # ---- edits of the coordinate sequences (gpk_seqedit.hip) ---------------------------------------------
    def segmentize(self, max_segment_length) -> "GeoSeries":
        """Every segment longer than `max_segment_length` split into ceil(len / max) equal pieces (gpk_segmentize; GeoPandas'
        segmentize, geo's Densify), as a device-resident series of the same type.  A scalar > 0, or one value per row (a row whose
        value is NaN or <= 0 stays as it is).  New coordinates are p + (q - p) * (j / n); the original ones are copied bit for bit."""
        m = segmentize_args("segmentize", self, max_segment_length)
        return GeoSeries(None, name=self.name, device=self.device().segmentize(m))

    def remove_repeated_points(self, tolerance: float = 0.0) -> "GeoSeries":
        """Consecutive equal coordinates of every linestring and ring dropped (gpk_remove_repeated_points).  Only tolerance == 0."""
        if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)) or not float(tolerance) == 0.0:
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"remove_repeated_points: only tolerance == 0 is implemented (found {tolerance!r})")
        return GeoSeries(None, name=self.name, device=self.device().remove_repeated_points(0.0))

    def reverse(self) -> "GeoSeries":
        """Every linestring and ring in reverse coordinate order (gpk_reverse); points are unchanged."""
        return GeoSeries(None, name=self.name, device=self.device().reverse())

    def orient_polygons(self, exterior_cw: bool = False) -> "GeoSeries":
        """Shells counter-clockwise and holes clockwise (RFC 7946), or the opposite with `exterior_cw` (gpk_orient_polygons): the
        exact turn at every ring's lexicographically smallest coordinate decides.  Other geometry types are copied."""
        if not isinstance(exterior_cw, (bool, np.bool_)):
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"orient_polygons: `exterior_cw` must be a bool (found {exterior_cw!r})")
        return GeoSeries(None, name=self.name, device=self.device().orient_polygons(bool(exterior_cw)))

    # ---- polygon x polygon union and the grouped union (gpk_polyunion.hip) ---------------------------
    def polygon_union(self, other: "GeoSeries", other_rows=None, return_status: bool = False):
        """The area every row's polygon or other[other_rows[i]] covers (gpk_polygon_union), as a MULTIPOLYGON series: neighbours that
        share an edge merge across it, rows that only touch at points stay separate parts, a hole goes to the innermost shell around
        it.  A null row where `polygon_intersection` gives one — also where either row has no coordinate: an empty row is not the
        neutral element here (`union_all` drops such rows first).  Coordinates, status and shapes as `polygon_intersection`."""
        return self._polygon_clip("polygon_union", _abi.PUNION_UNION, other, other_rows, return_status, entry="gpk_polygon_union")

    # ---- polygon x polygon symmetric difference (gpk_polysymdiff.hip) ---------------------------------
    def polygon_symmetric_difference(self, other: "GeoSeries", other_rows=None, return_status: bool = False):
        """The area exactly one of every row's polygon and other[other_rows[i]] covers (gpk_polygon_symdiff), as a MULTIPOLYGON
        series: GeoPandas' symmetric_difference on polygon columns, the area part only.  Equal polygons give a valid row without
        parts, neighbours that share an edge their union, a polygon strictly inside the other a hole (to the innermost shell around
        it); where the boundaries cross, a \\ b and b \\ a touch at the crossing and stay separate rings.  A null row where
        `polygon_union` gives one — an empty row is not the neutral element.  Coordinates, status and shapes as
        `polygon_intersection`."""
        return self._polygon_clip("polygon_symmetric_difference", _abi.PSYMDIFF_SYMMETRIC_DIFFERENCE, other, other_rows, return_status,
                                  entry="gpk_polygon_symdiff")

    def union_all(self, by=None, return_status: bool = False):
        """The union of the polygons of every group, one MULTIPOLYGON row per group in ascending group id (GeoPandas union_all /
        dissolve); `by`: an integer array, one entry per row (None: one group).  A tree reduction over gpk_polygon_union: rows that
        are null or have no coordinate are dropped first (a group with none left gives an EMPTY row, not null); each round unites
        rows 2i and 2i + 1 of every group's current list, an odd last row passes through, for ceil(log2(largest group)) rounds.  The
        pairing of a round is made on the device (gpk_union_all_pairs); the rounds' results are appended to a device-resident pool
        column (gpk_geoarray_concat) that the next round's row lists index, and nothing but two counts a round leaves the device.
        Every result row leaves through one last union of the row with itself, which returns its own coordinates.  With
        `return_status`: (series, status), the worst status a group met (uint8; 0 OK, 1 some ring touches itself, 2 an empty group,
        3 / 4 a null row: an invalid ring, or a round that did not resolve).  A status-1 intermediate is fed onward as it is: the
        result is then whatever gpk_polygon_union says for such input."""
        groups, n_groups = union_all_groups(self, by)
        host = self.array
        rows0 = _union_all_live_rows(host, groups)
        status = np.full(n_groups, _abi.PCLIP_EMPTY, dtype=np.uint8)
        z = np.zeros(1, dtype=np.int32)
        empty = GeoArrowArray(_abi.GEOM_MULTIPOLYGON, np.zeros((0, 2)), geom_offsets=np.zeros(n_groups + 1, dtype=np.int32), part_offsets=z,
                              ring_offsets=z.copy(), n_geoms=n_groups)
        if len(rows0) == 0:
            out = GeoSeries(empty)
            return (out, status) if return_status else out
        import torch

        lib = _abi.lib()
        pool = DeviceGeoArray.upload(_as_multipolygon(host.take(rows0)))
        dev = torch.device("cuda")
        group = torch.from_numpy(groups[rows0].astype(np.int32)).to(dev)
        rows, pool_status = None, torch.zeros(len(rows0), dtype=torch.uint8, device=dev)
        counts = (C.c_int64 * 2)()
        while True:
            n = group.shape[0]
            a_rows, b_rows = (torch.empty(max(n // 2, 1), dtype=torch.int32, device=dev) for _ in range(2))
            next_group, next_rows = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
            _abi.check(lib.gpk_union_all_pairs(group.data_ptr(), None if rows is None else rows.data_ptr(), n, pool.n_geoms, a_rows.data_ptr(),
                                               b_rows.data_ptr(), next_group.data_ptr(), next_rows.data_ptr(), counts, None))
            n_pairs, n_next = int(counts[0]), int(counts[1])
            if n_pairs == 0:
                break
            a_rows, b_rows = a_rows[:n_pairs], b_rows[:n_pairs]
            st = torch.empty(n_pairs, dtype=torch.uint8, device=dev)
            united = polygon_clip_call(pool, pool, a_rows.data_ptr(), b_rows.data_ptr(), n_pairs, _abi.MEM_DEVICE, _abi.PUNION_UNION, 0, None,
                                       _abi.MEM_DEVICE, st.data_ptr(), _abi.MEM_DEVICE, entry="gpk_polygon_union")
            st = torch.maximum(st, torch.maximum(pool_status[a_rows.long()], pool_status[b_rows.long()]))
            pool_status = torch.cat([pool_status, st])
            pool, _bases = DeviceGeoArray.concat([pool, united.device()])
            group, rows = next_group[:n_next], next_rows[:n_next]
        if rows is None:
            rows = torch.arange(group.shape[0], dtype=torch.int32, device=dev)
        n = rows.shape[0]
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        last = polygon_clip_call(pool, pool, rows.data_ptr(), rows.data_ptr(), n, _abi.MEM_DEVICE, _abi.PUNION_UNION, 0, None, _abi.MEM_DEVICE,
                                 st.data_ptr(), _abi.MEM_DEVICE, entry="gpk_polygon_union").array
        present = group.cpu().numpy()
        status[present] = torch.maximum(st, pool_status[rows.long()]).cpu().numpy()
        parts = np.zeros(n_groups, dtype=np.int64)
        parts[present] = np.diff(last.geom_offsets)
        valid = np.ones(n_groups, dtype=bool)
        valid[present] = status[present] < _abi.PCLIP_NULL
        out = GeoSeries(GeoArrowArray(_abi.GEOM_MULTIPOLYGON, last.xy, geom_offsets=np.concatenate([[0], np.cumsum(parts)]).astype(np.int32),
                                      part_offsets=last.part_offsets, ring_offsets=last.ring_offsets,
                                      validity=None if valid.all() else np.packbits(valid, bitorder="little"), n_geoms=n_groups))
        return (out, status) if return_status else out

    # ---- line x line relations (gpk_lineline.hip) ------------------------------------------------
    def line_relation(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """The exact relation mask (uint8) of every row's line A against its line B = other[other_rows[i]] (gpk_line_relation), under
        the mod-2 boundary rule: bit 1 — the interiors share a point, 2 — A and B share a piece of positive length, 4 — an interior
        point of A is a boundary point of B, 8 — a boundary point of A is an interior point of B, 16 — the boundaries share a point,
        32 — A has a point off B, 64 — B has a point off A; 0 for a null row, a row without coordinates or one with a NaN or infinite
        coordinate.  Both columns are LINESTRING / MULTILINESTRING.  The named methods (crosses, touches, ...) do not take two lineal
        columns: line_predicate does."""
        rows = line_relation_args("line_relation", self, other, other_rows)
        return self._rowwise("gpk_line_relation", self, other, rows, np.empty(len(self), dtype=np.uint8))

    def line_predicate(self, other: "GeoSeries", name: str, other_rows=None) -> np.ndarray:
        """a named line / line predicate (LINE_MASK_PREDICATES: intersects, disjoint, touches, crosses, overlaps, within, contains,
        covered_by, covers, equals) of every row against its row of `other`, as bool"""
        if name not in LINE_MASK_PREDICATES:
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"unknown line / line predicate {name!r}: one of {sorted(LINE_MASK_PREDICATES)}")
        return line_mask_predicate(self.line_relation(other, other_rows), name)

    # ---- point relations (gpk_pointrel.hip) ------------------------------------------------------
    def point_relation(self, other: "GeoSeries", other_rows=None) -> np.ndarray:
        """The exact relation mask (uint8) of every row's point set A against its geometry B (gpk_point_relation): bit 1 — a point of A
        lies in B's interior, 2 — on B's boundary (a ring of a polygon, a mod-2 end of a line; points have none), 4 — a point of A is
        no point of B, 8 — B has a point that is no point of A; 0 for a null or empty row, a NaN or infinite coordinate or an invalid
        ring.  One side is a POINT / MULTIPOINT column, the other any family, in either order; the punctual side is A (`self` when
        both are).  `other_rows` pairs row i with other[other_rows[i]] and needs `self` to be the punctual side."""
        points_first = point_relation_sides("point_relation", self._family(), other._family())
        rows = point_relation_rows_arg("point_relation", self, other, other_rows, points_first)
        points, geoms = (self, other) if points_first else (other, self)
        return self._rowwise("gpk_point_relation", points, geoms, rows, np.empty(len(points), dtype=np.uint8))

    def point_predicate(self, other: "GeoSeries", name: str, other_rows=None) -> np.ndarray:
        """a named predicate "self[i] NAME other[i]" with a POINT / MULTIPOINT column on either side (POINT_MASK_PREDICATES: intersects,
        disjoint, within, covered_by, contains, covers, contains_properly, touches, equals, crosses, overlaps), as bool; with the
        punctual column in `other` the name is transposed (within <-> contains, covered_by <-> covers)"""
        if name not in POINT_MASK_PREDICATES:
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"unknown point predicate {name!r}: one of {sorted(POINT_MASK_PREDICATES)}")
        points_first = point_relation_sides("point_predicate", self._family(), other._family())
        dim_b = family_dim(other._family() if points_first else self._family())
        return point_mask_predicate(self.point_relation(other, other_rows), name if points_first else point_transposed(name), dim_b)

    def predicate(self, other: "GeoSeries", name: str, other_rows=None) -> np.ndarray:
        """"self[i] NAME other[i]" for any two families, as bool: the relation family that serves the pair decides (predicate_route:
        point_predicate when either side is punctual, line_predicate for two line columns, the polygon relations for two polygon
        columns, the line / polygon relations otherwise), with that family's names.  The named methods (touches, crosses, ...) keep
        their own, narrower family pairs."""
        route, names = predicate_route(self._family(), other._family())
        if name not in names:
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"predicate: unknown {route} predicate {name!r}: one of {sorted(names)}")
        if route == "point":
            return self.point_predicate(other, name, other_rows)
        if route == "line":
            return self.line_predicate(other, name, other_rows)
        if route == "polygon":
            return self._polygon_relation(other, name, other_rows)
        return self._relation(other, name, other_rows)

    # ---- validity and simplicity (gpk_validity.hip) ----------------------------------------------
    def _validity(self, op: str, return_where: bool):
        validity_family_arg(op, self._family(), POLYGONAL)
        n = len(self)
        code = np.empty(n, dtype=np.uint8)
        where = np.empty(n, dtype=np.int32) if return_where else None
        if n:
            _abi.check(_abi.lib().gpk_validity(self.device().handle, code.ctypes.data, where.ctypes.data if return_where else None, MEM_HOST, None))
        return code, where

    def is_valid_reason(self, return_where: bool = False):
        """Why a polygon row is not OGC-valid (gpk_validity): one uint8 code per row, 0 for a valid row — VALIDITY_NAMES[code] names
        it; the lowest code that applies.  With `return_where` also the int32 index, in the column's coordinate buffer, of the
        coordinate, segment, ring or member at fault (-1 for valid and null rows).  A POLYGON or MULTIPOLYGON column."""
        code, where = self._validity("is_valid_reason", return_where)
        return (code, where) if return_where else code

    def is_valid(self) -> np.ndarray:
        """GeoPandas' GeoSeries.is_valid for a POLYGON or MULTIPOLYGON column: True where the relation masks are exact for the row
        (is_valid_reason gives code 0; a row without a non-empty member is valid, a null row is not)"""
        return self._validity("is_valid", False)[0] == 0

    def is_simple(self) -> np.ndarray:
        """GeoPandas' GeoSeries.is_simple for a LINESTRING or MULTILINESTRING column (gpk_is_simple): no member meets itself except a
        closed one at its start, and two members share only common end points; False for null rows and non-finite coordinates"""
        validity_family_arg("is_simple", self._family(), LINEAL)
        out = np.empty(len(self), dtype=np.uint8)
        if len(out):
            _abi.check(_abi.lib().gpk_is_simple(self.device().handle, out.ctypes.data, MEM_HOST, None))
        return out.astype(bool)

    # ---- triangulation (gpk_triangulate.hip) -------------------------------------------------------
    def triangulate(self, return_status: bool = False):
        """Every row of a POLYGON or MULTIPOLYGON column as triangles over the column's own coordinate buffer (gpk_triangulate: exact
        ear clipping, holes bridged, touching rings split): (tri_offsets int32[n + 1], tri_index uint32[T, 3]) — row i owns triangles
        tri_offsets[i] .. tri_offsets[i + 1], each three indices into the coordinate buffer, counter-clockwise.  With `return_status`
        also the uint8 TRIANGULATE_STATUS code per row: 0 triangulated, 1 null or empty, 2 failed (an invalid row: see is_valid)."""
        validity_family_arg("triangulate", self._family(), POLYGONAL)
        return_status = bool_arg("triangulate", "return_status", return_status)
        n = len(self)
        offsets = np.zeros(n + 1, dtype=np.int32)
        status = np.empty(n, dtype=np.uint8)
        total = C.c_int64(0)
        index = np.empty((0, 3), dtype=np.uint32)
        if n:
            h = self.device().handle
            _abi.check(_abi.lib().gpk_triangulate(h, None, 0, offsets.ctypes.data, status.ctypes.data, C.byref(total), MEM_HOST, None))
            index = np.empty((int(total.value), 3), dtype=np.uint32)
            if len(index):
                _abi.check(_abi.lib().gpk_triangulate(h, index.ctypes.data, len(index), offsets.ctypes.data, status.ctypes.data, C.byref(total), MEM_HOST, None))
        return (offsets, index, status) if return_status else (offsets, index)

    def triangles(self, return_parents: bool = False):
        """The triangles of triangulate() as a POLYGON series: one row per triangle, each a closed counter-clockwise ring of four
        coordinates that are the input's bit for bit (gathered on the device).  With `return_parents` also the int32 row each triangle
        came from, as in explode."""
        return_parents = bool_arg("triangles", "return_parents", return_parents)
        offsets, index = self.triangulate()
        import torch

        xy = torch.from_numpy(self.array.xy).cuda()
        corners = torch.from_numpy(index.astype(np.int64)).cuda()[:, [0, 1, 2, 0]]
        rings = xy[corners.reshape(-1)].cpu().numpy().reshape(-1, 2)
        t = len(index)
        out = GeoSeries(GeoArrowArray(GEOM_POLYGON, rings, geom_offsets=np.arange(t + 1, dtype=np.int32), ring_offsets=np.arange(0, 4 * t + 1, 4, dtype=np.int32)))
        if not return_parents:
            return out
        return out, np.repeat(np.arange(len(self), dtype=np.int32), np.diff(offsets))

    # ---- linear referencing (gpk_linref.hip) -----------------------------------------------------
    def _family(self) -> int:
        return self._dev.geom_type if self._array is None else self._array.geom_type

    def closest_point(self, other: "GeoSeries", other_rows=None, return_segment: bool = False):
        """geo's ClosestPoint / shapely's nearest_points: for every point of `self` (a POINT column) the nearest point of
        other[other_rows[i]] (any family), as a POINT series; null where there is none (a null or empty row, a NaN point).  A point
        inside or on a polygon is its own closest point.  With `return_segment` also the int32 index, in `other`'s coordinate
        buffer, of the start of the segment the point lies on (the lowest one among ties; -1: none, or inside a polygon)."""
        rows = linref_args("closest_point", self, other, other_rows)
        n = len(self)
        xy = np.empty((n, 2), dtype=np.float64)
        seg = np.empty(n, dtype=np.int32) if return_segment else None
        if n:
            _abi.check(
                _abi.lib().gpk_closest_point_rowwise(
                    self.device().handle, other.device().handle, None if rows is None else rows.ctypes.data, xy.ctypes.data,
                    seg.ctypes.data if return_segment else None, MEM_HOST, None,
                )
            )
        ok =~np.isnan(xy[:, 0])
        out = GeoSeries(GeoArrowArray.from_points(xy, validity=None if ok.all() else np.packbits(ok, bitorder="little")))
        return (out, seg) if return_segment else out

    def shortest_line(self, other: "GeoSeries", other_rows=None) -> "GeoSeries":
        """shapely's shortest_line: the two-coordinate LINESTRING [p, closest_point(p)] per row (assembled on the host from
        closest_point); null where there is no closest point."""
        q = self.closest_point(other, other_rows)
        n = len(self)
        xy = np.empty((2 * n, 2), dtype=np.float64)
        xy[0::2] = self.array.xy
        xy[1::2] = q.array.xy
        return GeoSeries(GeoArrowArray(GEOM_LINESTRING, xy, geom_offsets=np.arange(0, 2 * n + 1, 2, dtype=np.int32), validity=q.array.validity, n_geoms=n))

    def project(self, other: "GeoSeries", normalized: bool = False, rows=None) -> np.ndarray:
        """GeoPandas' GeoSeries.project / geo's LineLocatePoint: `self` is a LINESTRING or MULTILINESTRING column, `other` a POINT
        column; one result per point: the distance along self[rows[i]] (default: self[i]) of its point nearest to other[i], as a
        fraction of the line's length with `normalized`.  A MULTILINESTRING's members are measured one after the other.  NaN for
        null and empty rows and NaN points."""
        r = linref_args("project", other, self, rows, lineal_only=True)
        return self._rowwise("gpk_line_locate_point", other, self, r, np.empty(len(other), dtype=np.float64), int(bool(normalized)))

    def interpolate(self, distance, normalized: bool = False) -> "GeoSeries":
        """GeoPandas' GeoSeries.interpolate / geo's LineInterpolatePoint: the point at `distance` (a number, or one per row) along each
        LINESTRING or MULTILINESTRING; a negative distance is taken from the end, one beyond either end gives that end; with
        `normalized` a fraction of the line's length.  Null for null and empty rows and NaN distances."""
        d = interpolate_distance_arg(self, distance)
        n = len(self)
        xy = np.empty((n, 2), dtype=np.float64)
        valid = np.ones(n, dtype=np.uint8)
        if n:
            _abi.check(
                _abi.lib().gpk_line_interpolate_point(
                    self.device().handle, d.ctypes.data, len(d), int(bool(normalized)), xy.ctypes.data, valid.ctypes.data, MEM_HOST, None
                )
            )
        ok = valid.astype(bool)
        return GeoSeries(GeoArrowArray.from_points(xy, validity=None if ok.all() else np.packbits(ok, bitorder="little")))


def _mismatch(msg: str) -> "_abi.MismatchedGeometry":
    return _abi.MismatchedGeometry(_abi.GPK_ERR_MISMATCHED_GEOMETRY, msg)


def linref_args(op: str, points: GeoSeries, other: GeoSeries, rows, lineal_only: bool = False) -> Optional[np.ndarray]:
    """the checks of closest_point / project, before any device call: `points` is a POINT column, `other` lineal where the operator
    needs it, the row map (as uint32, or None) pairs every point with a row; refusals as the C ABI would make them"""
    if points._family() != GEOM_POINT:
        raise _mismatch(f"{op}: the point side must be POINT (found {_abi_name(points._family())})")
    if lineal_only and other._family() not in (GEOM_LINESTRING, GEOM_MULTILINESTRING):
        raise _mismatch(f"{op}: expected LineString or MultiLineString (found {_abi_name(other._family())})")
    return paired_rows_arg(op, points, other, rows, "points")


def row_map_arg(op: str, rows, n: int, what: str = "rows") -> np.ndarray:
    """a caller's row map as the library gets it: a contiguous 1-D uint32 array of `n` row numbers, one per row (`what`: the noun of the
    message) of the mapped side; anything else is refused here, before any device call"""
    try:
        r = np.ascontiguousarray(rows, dtype=np.uint32)
    except (TypeError, ValueError, OverflowError):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: the row map must be an array of row numbers") from None
    if r.ndim != 1 or len(r) != n:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: {r.size} row numbers for {n} {what}")
    return r


def paired_rows_arg(op: str, a: GeoSeries, b: GeoSeries, rows, what: str = "rows") -> Optional[np.ndarray]:
    """the row pairing of a row-wise operator before any device call: without a row map the row counts match (None); a row map has one
    entry per row of `a` (row_map_arg)"""
    if rows is None:
        if len(a) != len(b):
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: row counts differ ({len(a)} vs {len(b)})")
        return None
    return row_map_arg(op, rows, len(a), what)


def either_order_rows_arg(op: str, a: GeoSeries, b: GeoSeries, rows, mapped_first: bool, needs: str) -> Optional[np.ndarray]:
    """the row pairing of a relation that takes its two families in either order: as paired_rows_arg, but a row map needs the side it
    maps from on the left (`mapped_first`) unless it is the identity, which then counts as no map; `needs` says so in the refusal"""
    if rows is not None:
        r = row_map_arg(op, rows, len(a))
        if mapped_first:
            return r
        if not np.array_equal(r, np.arange(len(a), dtype=np.uint32)):
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: {needs}")
    return paired_rows_arg(op, a, b, None)


def interpolate_distance_arg(lines: GeoSeries, distance) -> np.ndarray:
    """the `distance` of interpolate as a float64 array of 1 value (a scalar: it stays one value) or len(lines) values; a wrong
    family, length or anything not convertible to float is refused here, before any device call"""
    if lines._family() not in (GEOM_LINESTRING, GEOM_MULTILINESTRING):
        raise _mismatch(f"interpolate: expected LineString or MultiLineString (found {_abi_name(lines._family())})")
    try:
        if distance is None:
            raise TypeError("None")
        d = np.asarray(distance, dtype=np.float64)
    except (TypeError, ValueError):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"interpolate: distance must be a number or an array of numbers, got {distance!r}") from None
    if d.ndim == 0:
        return d.reshape(1)
    if d.ndim != 1 or len(d) != len(lines):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"interpolate: {d.size} distances for {len(lines)} rows (a scalar or one per row)")
    return np.ascontiguousarray(d)


LINEAL = (GEOM_LINESTRING, GEOM_MULTILINESTRING)
POLYGONAL = (GEOM_POLYGON, GEOM_MULTIPOLYGON)

# the line / area predicates over the relation mask (include/geopolars_hip.h); mask 0 — an unusable row — satisfies none of them
MASK_PREDICATES = {
    "intersects": lambda m: (m & 3) != 0,
    "disjoint": lambda m: m == 4,
    "covered_by": lambda m: (m != 0) & ((m & 4) == 0),
    "within": lambda m: ((m & 1) != 0) & ((m & 4) == 0),
    "crosses": lambda m: ((m & 1) != 0) & ((m & 4) != 0),
    "touches": lambda m: ((m & 2) != 0) & ((m & 1) == 0),
}
MASK_PREDICATES["covers"] = MASK_PREDICATES["covered_by"]  # the polygon's view of the same relation
MASK_PREDICATES["contains"] = MASK_PREDICATES["within"]


def mask_predicate(mask, name: str) -> np.ndarray:
    """a named line / polygon predicate from relation masks"""
    if name not in MASK_PREDICATES:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"unknown line / polygon predicate {name!r}: one of {sorted(MASK_PREDICATES)}")
    return MASK_PREDICATES[name](np.asarray(mask, dtype=np.uint8))


# the area / area predicates over the polygon x polygon relation mask (include/geopolars_hip.h); mask 0 satisfies none of them
POLYGON_MASK_PREDICATES = {
    "intersects": lambda m: (m & 3) != 0,
    "disjoint": lambda m: (m != 0) & ((m & 3) == 0),
    "touches": lambda m: ((m & 2) != 0) & ((m & 1) == 0),
    "overlaps": lambda m: (m & 13) == 13,
    "within": lambda m: ((m & 1) != 0) & ((m & 4) == 0),
    "contains": lambda m: ((m & 1) != 0) & ((m & 8) == 0),
    "equals": lambda m: ((m & 1) != 0) & ((m & 12) == 0),
    "contains_properly": lambda m: (m & 11) == 1,
    "crosses": lambda m: np.zeros(m.shape, dtype=bool),  # two areas never cross
}
POLYGON_MASK_PREDICATES["covered_by"] = POLYGON_MASK_PREDICATES["within"]  # closed regular sets: covered means within
POLYGON_MASK_PREDICATES["covers"] = POLYGON_MASK_PREDICATES["contains"]


# the line / line predicates over the line x line relation mask (include/geopolars_hip.h); mask 0 satisfies none of them
LINE_MASK_PREDICATES = {
    "intersects": lambda m: (m & 31) != 0,
    "disjoint": lambda m: (m != 0) & ((m & 31) == 0),
    "touches": lambda m: ((m & 28) != 0) & ((m & 1) == 0),
    "crosses": lambda m: ((m & 1) != 0) & ((m & 2) == 0),
    "overlaps": lambda m: ((m & 2) != 0) & ((m & 32) != 0) & ((m & 64) != 0),
    "within": lambda m: ((m & 1) != 0) & ((m & 32) == 0),
    "contains": lambda m: ((m & 1) != 0) & ((m & 64) == 0),
    "covered_by": lambda m: ((m & 31) != 0) & ((m & 32) == 0),
    "covers": lambda m: ((m & 31) != 0) & ((m & 64) == 0),
    "equals": lambda m: ((m & 1) != 0) & ((m & 96) == 0),
}


def line_mask_predicate(mask, name: str) -> np.ndarray:
    """a named line / line predicate from relation masks"""
    if name not in LINE_MASK_PREDICATES:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"unknown line / line predicate {name!r}: one of {sorted(LINE_MASK_PREDICATES)}")
    return LINE_MASK_PREDICATES[name](np.asarray(mask, dtype=np.uint8))


def line_relation_args(op: str, a: "GeoSeries", b: "GeoSeries", rows) -> Optional[np.ndarray]:
    """the checks of line_relation before any device call, in the C ABI's order: both families lineal, then the row map (returned as
    uint32) with one entry per row of `a`, or equal row counts without one"""
    fa, fb = a._family(), b._family()
    if fa not in LINEAL or fb not in LINEAL:
        raise _mismatch(f"{op}: LineString | MultiLineString x LineString | MultiLineString (found {_abi_name(fa)} x {_abi_name(fb)})")
    return paired_rows_arg(op, a, b, rows)


PUNCTUAL = (GEOM_POINT, GEOM_MULTIPOINT)


def family_dim(t: int) -> int:
    """the dimension of a geometry family: 0 punctual, 1 lineal, 2 polygonal; any other type is refused"""
    if t in PUNCTUAL:
        return 0
    if t in LINEAL:
        return 1
    if t in POLYGONAL:
        return 2
    raise _mismatch(f"no relation is defined for geometry type {t}")


# the point predicates over the point relation mask and the dimension of B's family (include/geopolars_hip.h); mask 0 satisfies none
POINT_MASK_PREDICATES = {
    "intersects": lambda m, d: (m & 3) != 0,
    "disjoint": lambda m, d: (m != 0) & ((m & 3) == 0),
    "within": lambda m, d: ((m & 1) != 0) & ((m & 4) == 0),
    "covered_by": lambda m, d: ((m & 3) != 0) & ((m & 4) == 0),
    "contains": lambda m, d: ((m & 1) != 0) & ((m & 8) == 0),
    "covers": lambda m, d: ((m & 3) != 0) & ((m & 8) == 0),
    "touches": lambda m, d: ((m & 2) != 0) & ((m & 1) == 0),
    "equals": lambda m, d: ((m & 1) != 0) & ((m & 12) == 0),
    "crosses": lambda m, d: ((m & 1) != 0) & ((m & 4) != 0) if d >= 1 else np.zeros(m.shape, dtype=bool),
    "overlaps": lambda m, d: (m & 13) == 13 if d == 0 else np.zeros(m.shape, dtype=bool),
}
POINT_MASK_PREDICATES["contains_properly"] = POINT_MASK_PREDICATES["contains"]  # a point set has no boundary to touch
# "B contains_properly A" has no name of its own read from A: every point of A in B's interior, none on its boundary
POINT_TRANSPOSED = {"within": "contains", "contains": "within", "covered_by": "covers", "covers": "covered_by", "contains_properly": "properly_within"}
_POINT_TRANSPOSED_ONLY = {"properly_within": lambda m, d: (m & 7) == 1}


def point_transposed(name: str) -> str:
    """"B NAME A" as a predicate of (A, B), A the punctual side: within <-> contains, covered_by <-> covers, the rest read the same"""
    return POINT_TRANSPOSED.get(name, name)


def point_mask_predicate(mask, name: str, dim_b: int) -> np.ndarray:
    """a named point predicate from relation masks; dim_b: the dimension of B's family (0, 1, 2)"""
    f = POINT_MASK_PREDICATES.get(name) or _POINT_TRANSPOSED_ONLY.get(name)
    if f is None:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"unknown point predicate {name!r}: one of {sorted(POINT_MASK_PREDICATES)}")
    if dim_b not in (0, 1, 2):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"point predicate: the dimension of B's family must be 0, 1 or 2 (found {dim_b!r})")
    return f(np.asarray(mask, dtype=np.uint8), dim_b)


def point_relation_sides(op: str, a: int, b: int) -> bool:
    """True when family `a` is punctual (A = the left column, also when both are), False when only `b` is; any other pair is refused as
    the C ABI would"""
    known = PUNCTUAL + LINEAL + POLYGONAL
    if a in PUNCTUAL and b in known:
        return True
    if b in PUNCTUAL and a in known:
        return False
    raise _mismatch(f"{op}: Point | MultiPoint x any family, in either order (found {_abi_name(a)} x {_abi_name(b)})")


def point_relation_rows_arg(op: str, a: "GeoSeries", b: "GeoSeries", rows, points_first: bool) -> Optional[np.ndarray]:
    """the checks of point_relation before any device call: without a row map the row counts match; a row map (returned as uint32) has
    one entry per row of `a` and needs `a` to be the punctual side unless it is the identity"""
    return either_order_rows_arg(op, a, b, rows, points_first, "a row map needs the punctual column on the left (it maps point rows to rows of the other column)")


def predicate_route(a: int, b: int):
    """(the relation family that serves the pair of geometry types — "point", "line", "polygon" or "line_polygon" — and its predicate
    names): the dispatch table of GeoSeries.predicate and spatial_index.sjoin; an unknown type is refused"""
    da, db = family_dim(a), family_dim(b)
    if da == 0 or db == 0:
        return "point", POINT_MASK_PREDICATES
    if da == 1 and db == 1:
        return "line", LINE_MASK_PREDICATES
    if da == 2 and db == 2:
        return "polygon", POLYGON_MASK_PREDICATES
    return "line_polygon", MASK_PREDICATES


# the codes of gpk_validity (include/geopolars_hip.h: GPK_VALID, GPK_INVALID_*), by value
VALIDITY_NAMES = (
    "valid",
    "invalid coordinate",
    "invalid ring shape",
    "ring self-intersection",
    "rings cross",
    "hole outside shell",
    "nested holes",
    "nested members",
    "disconnected interior",
    "null",
)


def return_width_arg(return_width) -> bool:
    """the `return_width` of representative_point as a bool; anything else is refused here, before any device call"""
    if not isinstance(return_width, (bool, np.bool_)):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"representative_point: return_width must be a bool (found {return_width!r})")
    return bool(return_width)


def representative_point_device(dev: DeviceGeoArray, out_xy, out_valid=None, out_width=None, stream: int = 0) -> DeviceGeoArray:
    """Device-buffer variant of representative_point: out_xy (n, 2) float64, out_valid (n,) uint8 and out_width (n,) float64 torch
    CUDA tensors (the last two optional) are filled in place on `stream`.  Returns a POINT DeviceGeoArray that views out_xy — rows
    without an answer are NaN points, which every join treats as empty — so the result feeds a join without a host round trip."""
    if not isinstance(dev, DeviceGeoArray):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, "representative_point_device: a DeviceGeoArray is needed")
    n = dev.n_geoms
    for name, t, shape, dtype in (("out_xy", out_xy, (n, 2), "torch.float64"), ("out_valid", out_valid, (n,), "torch.uint8"),
                                  ("out_width", out_width, (n,), "torch.float64")):
        if t is None and name != "out_xy":
            continue
        if t is None or tuple(getattr(t, "shape", ())) != shape or str(getattr(t, "dtype", None)) != dtype or not t.is_cuda or not t.is_contiguous():
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"representative_point_device: {name} must be a contiguous CUDA tensor of shape {shape}, {dtype}")
    if n:
        _abi.check(_abi.lib().gpk_representative_point(
            dev.handle, out_xy.data_ptr(), None if out_valid is None else out_valid.data_ptr(), None if out_width is None else out_width.data_ptr(),
            _abi.MEM_DEVICE, stream))
    return DeviceGeoArray.from_device_buffers(GEOM_POINT, out_xy, stream=stream)


def _ring_series(xy: np.ndarray, ok: np.ndarray, k: int, validity) -> GeoSeries:
    """a POLYGON series of one k-coordinate ring per row with ok, an empty polygon (no ring) per row without; `validity` is the input's"""
    n = len(ok)
    xy = np.ascontiguousarray(xy.reshape(n, k, 2)[ok].reshape(-1, 2))
    geom_off = np.concatenate(([0], np.cumsum(ok, dtype=np.int64))).astype(np.int32)
    ring_off = np.arange(0, k * int(ok.sum()) + 1, k, dtype=np.int32)
    return GeoSeries(GeoArrowArray(GEOM_POLYGON, xy, geom_offsets=geom_off, ring_offsets=ring_off, validity=validity, n_geoms=n))


def quad_segs_arg(quad_segs) -> int:
    """the `quad_segs` of minimum_bounding_circle as an int in 1 .. 256; anything else is refused here, before any device call"""
    if isinstance(quad_segs, (bool, np.bool_)) or not isinstance(quad_segs, (int, np.integer)) or not 1 <= int(quad_segs) <= 256:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"minimum_bounding_circle: quad_segs must be an integer in 1 .. 256 (found {quad_segs!r})")
    return int(quad_segs)


def circle_rings(centre: np.ndarray, radius: np.ndarray, quad_segs: int) -> np.ndarray:
    """(n * (4 quad_segs + 1), 2): per row centre + r (cos t, sin t) for t = 0, pi / (2 quad_segs), ... counter-clockwise, closed by a copy
    of the first coordinate"""
    m = 4 * quad_segs
    t = np.arange(m, dtype=np.float64) * (np.pi / (2 * quad_segs))
    ring = np.empty((len(radius), m + 1, 2), dtype=np.float64)
    ring[:, :m, 0] = centre[:, 0:1] + radius[:, None] * np.cos(t)[None, :]
    ring[:, :m, 1] = centre[:, 1:2] + radius[:, None] * np.sin(t)[None, :]
    ring[:, m] = ring[:, 0]
    return ring.reshape(-1, 2)


def _device_out_args(op: str, dev, outs):
    """the checks of the device-buffer forms before any device call: a DeviceGeoArray, and every given buffer a contiguous CUDA tensor of
    its shape and dtype (`outs`: (name, tensor, shape, dtype, required))"""
    if not isinstance(dev, DeviceGeoArray):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: a DeviceGeoArray is needed")
    for name, t, shape, dtype, required in outs(dev.n_geoms):
        if t is None and not required:
            continue
        if t is None or tuple(getattr(t, "shape", ())) != shape or str(getattr(t, "dtype", None)) != dtype or not t.is_cuda or not t.is_contiguous():
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: {name} must be a contiguous CUDA tensor of shape {shape}, {dtype}")


def minimum_rotated_rectangle_device(dev: DeviceGeoArray, out_xy, out_valid=None, stream: int = 0) -> None:
    """Device-buffer variant of minimum_rotated_rectangle: out_xy (n, 5, 2) float64 and out_valid (n,) uint8 (optional) torch CUDA tensors
    are filled in place on `stream`; rows without an answer are NaN."""
    _device_out_args("minimum_rotated_rectangle_device", dev,
                     lambda n: (("out_xy", out_xy, (n, 5, 2), "torch.float64", True), ("out_valid", out_valid, (n,), "torch.uint8", False)))
    if dev.n_geoms:
        _abi.check(_abi.lib().gpk_minimum_rotated_rectangle(
            dev.handle, out_xy.data_ptr(), None if out_valid is None else out_valid.data_ptr(), _abi.MEM_DEVICE, stream))


def minimum_bounding_circle_device(dev: DeviceGeoArray, out_radius, out_center=None, out_valid=None, stream: int = 0) -> None:
    """Device-buffer variant of minimum_bounding_circle_parts: out_radius (n,) float64, out_center (n, 2) float64 and out_valid (n,) uint8
    torch CUDA tensors (the last two optional) are filled in place on `stream`; rows without an answer are NaN."""
    _device_out_args("minimum_bounding_circle_device", dev,
                     lambda n: (("out_radius", out_radius, (n,), "torch.float64", True), ("out_center", out_center, (n, 2), "torch.float64", False),
                                ("out_valid", out_valid, (n,), "torch.uint8", False)))
    if dev.n_geoms:
        _abi.check(_abi.lib().gpk_minimum_bounding_circle(
            dev.handle, None if out_center is None else out_center.data_ptr(), out_radius.data_ptr(),
            None if out_valid is None else out_valid.data_ptr(), _abi.MEM_DEVICE, stream))


def bool_arg(op: str, name: str, value) -> bool:
    """a flag of triangulate / triangles as a bool; anything else is refused here, before any device call"""
    if not isinstance(value, (bool, np.bool_)):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: {name} must be a bool (found {value!r})")
    return bool(value)


def geodesic_points_arg(op: str, a: GeoSeries, b: GeoSeries) -> None:
    """the geodesic point operators take POINT columns; anything else is refused here, before any device call"""
    for s in (a, b):
        if s.array.geom_type != GEOM_POINT:
            raise _mismatch(f"{op}: POINT columns are needed (found {_abi_name(s.array.geom_type)})")


def geodesic_values_arg(op: str, name: str, value, n: int) -> np.ndarray:
    """a bearing / distance argument as a contiguous f64 array of one value or of n; refused here, before any device call, otherwise"""
    try:
        v = np.ascontiguousarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: {name} must be a number or an array of numbers") from None
    if v.ndim == 0:
        v = v.reshape(1)
    if v.ndim != 1 or len(v) not in (1, n):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: {name} holds {v.size} values for {n} rows (one, or one a row)")
    return v


def geodesic_area_device(dev: DeviceGeoArray, out_area=None, out_perimeter=None, signed: bool = False, stream: int = 0) -> None:
    """Device-buffer variant of geodesic_area / geodesic_perimeter: out_area and out_perimeter (n,) float64 torch CUDA tensors (either
    may be None) are filled in place on `stream`."""
    _device_out_args("geodesic_area_device", dev,
                     lambda n: (("out_area", out_area, (n,), "torch.float64", False), ("out_perimeter", out_perimeter, (n,), "torch.float64", False)))
    flags = _abi.GEODESIC_AREA_SIGNED if bool_arg("geodesic_area_device", "signed", signed) else 0
    if dev.n_geoms:
        _abi.check(_abi.lib().gpk_geodesic_area(dev.handle, flags, None if out_area is None else out_area.data_ptr(),
                                                None if out_perimeter is None else out_perimeter.data_ptr(), _abi.MEM_DEVICE, stream))


def geodesic_inverse_device(dev: DeviceGeoArray, other: DeviceGeoArray, out_distance=None, out_bearing=None, out_final_bearing=None,
                            stream: int = 0) -> None:
    """Device-buffer variant of geodesic_distance / geodesic_bearing over two POINT columns of equally many rows: the (n,) float64 torch
    CUDA tensors given (any may be None) are filled in place on `stream`."""
    _device_out_args("geodesic_inverse_device", dev,
                     lambda n: (("out_distance", out_distance, (n,), "torch.float64", False), ("out_bearing", out_bearing, (n,), "torch.float64", False),
                                ("out_final_bearing", out_final_bearing, (n,), "torch.float64", False)))
    if not isinstance(other, DeviceGeoArray):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, "geodesic_inverse_device: a DeviceGeoArray is needed")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _abi.check(_abi.lib().gpk_geodesic_inverse(dev.handle, other.handle, None, ptr(out_distance), ptr(out_bearing), ptr(out_final_bearing),
                                               _abi.MEM_DEVICE, stream))


def geodesic_destination_device(dev: DeviceGeoArray, bearing, distance, out_xy, out_bearing=None, stream: int = 0) -> None:
    """Device-buffer variant of geodesic_destination: bearing and distance are float64 torch CUDA tensors of shape (1,) or (n,), out_xy
    (n, 2) and out_bearing (n,) (optional: the azimuth on arrival) are filled in place on `stream`."""
    _device_out_args("geodesic_destination_device", dev,
                     lambda n: (("out_xy", out_xy, (n, 2), "torch.float64", True), ("out_bearing", out_bearing, (n,), "torch.float64", False)))
    for name, t in (("bearing", bearing), ("distance", distance)):
        shape = tuple(getattr(t, "shape", ()))
        if shape not in ((1,), (dev.n_geoms,)) or str(getattr(t, "dtype", None)) != "torch.float64" or not t.is_cuda or not t.is_contiguous():
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT,
                                         f"geodesic_destination_device: {name} must be a contiguous CUDA float64 tensor of shape (1,) or ({dev.n_geoms},)")
    _abi.check(_abi.lib().gpk_geodesic_direct(dev.handle, bearing.data_ptr(), bearing.shape[0], distance.data_ptr(), distance.shape[0], out_xy.data_ptr(),
                                              None if out_bearing is None else out_bearing.data_ptr(), _abi.MEM_DEVICE, stream))


TRIANGULATE_STATUS = ("triangulated", "null or empty", "failed")


def triangulate_device(dev: DeviceGeoArray, out_index, out_offsets, out_status=None, stream: int = 0) -> int:
    """Device-buffer variant of triangulate: out_offsets (n + 1,) int32, out_status (n,) uint8 (optional) and out_index (capacity, 3)
    int32 (the u32 indices: a column has fewer than 2^31 coordinates) torch CUDA tensors are filled in place on `stream`; out_index
    None is the size query.  Returns the number
    of triangles; a capacity below it raises GPK_ERR_CAPACITY (n_coords + 3 n_rings always suffices).  One read-back: the total."""
    if not isinstance(dev, DeviceGeoArray):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, "triangulate_device: a DeviceGeoArray is needed")
    validity_family_arg("triangulate_device", dev.geom_type, POLYGONAL)
    n = dev.n_geoms

    def ok(t, shape, dtype):
        return t is not None and tuple(getattr(t, "shape", ())) == shape and str(getattr(t, "dtype", None)) == dtype and t.is_cuda and t.is_contiguous()

    if not ok(out_offsets, (n + 1,), "torch.int32"):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"triangulate_device: out_offsets must be a contiguous CUDA tensor of shape {(n + 1,)}, torch.int32")
    if out_status is not None and not ok(out_status, (n,), "torch.uint8"):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"triangulate_device: out_status must be a contiguous CUDA tensor of shape {(n,)}, torch.uint8")
    cap = 0
    if out_index is not None:
        shape = tuple(getattr(out_index, "shape", ()))
        if len(shape) != 2 or shape[1] != 3 or not ok(out_index, shape, "torch.int32"):
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, "triangulate_device: out_index must be a contiguous CUDA tensor of shape (capacity, 3), torch.int32")
        cap = shape[0]
    total = C.c_int64(0)
    _abi.check(_abi.lib().gpk_triangulate(dev.handle, None if out_index is None else out_index.data_ptr(), cap, out_offsets.data_ptr(),
                                          None if out_status is None else out_status.data_ptr(), C.byref(total), _abi.MEM_DEVICE, stream))
    return int(total.value)


def validity_family_arg(op: str, family: int, allowed) -> None:
    """the family check of is_valid / is_valid_reason / is_simple before any device call, refused as the C ABI would"""
    if family not in allowed:
        want = "Polygon | MultiPolygon" if allowed is POLYGONAL else "LineString | MultiLineString"
        raise _mismatch(f"{op}: {want} (found {_abi_name(family)})")


def polygon_mask_predicate(mask, name: str) -> np.ndarray:
    """a named polygon / polygon predicate from relation masks"""
    if name not in POLYGON_MASK_PREDICATES:
        raise _abi.GeopolarsHipError(
            _abi.GPK_ERR_INVALID_ARGUMENT, f"unknown polygon / polygon predicate {name!r}: one of {sorted(POLYGON_MASK_PREDICATES)}"
        )
    return POLYGON_MASK_PREDICATES[name](np.asarray(mask, dtype=np.uint8))


def polygon_relation_args(op: str, a: GeoSeries, b: GeoSeries, rows) -> Optional[np.ndarray]:
    """the checks of polygon_relation before any device call, in the C ABI's order: both families polygonal, then the row map (returned
    as uint32) with one entry per row of `a`, or equal row counts without one"""
    fa, fb = a._family(), b._family()
    if fa not in POLYGONAL or fb not in POLYGONAL:
        raise _mismatch(f"{op}: Polygon | MultiPolygon x Polygon | MultiPolygon (found {_abi_name(fa)} x {_abi_name(fb)})")
    return paired_rows_arg(op, a, b, rows)


def intersection_measure_args(op: str, first, a: GeoSeries, b: GeoSeries, rows) -> Optional[np.ndarray]:
    """the checks of intersection_area / intersection_length before any device call, in the C ABI's order: `a` of the family set
    `first` (POLYGONAL: the area, LINEAL: the length) and `b` polygonal, then the row map (returned as uint32) with one entry per row
    of `a`, or equal row counts without one"""
    fa, fb = a._family(), b._family()
    if fa not in first or fb not in POLYGONAL:
        want = "Polygon | MultiPolygon" if first is POLYGONAL else "LineString | MultiLineString"
        swap = ": the lines come first, swap the arguments" if first is LINEAL and fa in POLYGONAL and fb in LINEAL else ""
        raise _mismatch(f"{op}: {want} x Polygon | MultiPolygon (found {_abi_name(fa)} x {_abi_name(fb)}){swap}")
    return paired_rows_arg(op, a, b, rows)


def line_clip_args(op: str, a: GeoSeries, b: GeoSeries, rows) -> Optional[np.ndarray]:
    """the checks of intersection / difference before any device call: lines x polygons (the measures exist for the other families),
    then the row map as in intersection_measure_args"""
    fa, fb = a._family(), b._family()
    if fa not in LINEAL or fb not in POLYGONAL:
        swap = ": the lines come first, swap the arguments" if fa in POLYGONAL and fb in LINEAL else ""
        raise _mismatch(
            f"{op}: LineString | MultiLineString x Polygon | MultiPolygon (found {_abi_name(fa)} x {_abi_name(fb)}){swap}; the other "
            "families have intersection_area / intersection_length, not the geometry"
        )
    return intersection_measure_args(op, LINEAL, a, b, rows)


def line_clip_call(lines, polys, line_rows, poly_rows, n_rows: int, rows_space: int, mode: int, flags: int, out_src, src_space: int, stream=None) -> GeoSeries:
    """gpk_line_clip on two DeviceGeoArrays and raw row-list pointers: the owned MULTILINESTRING result as a device-resident series"""
    h = C.c_void_p()
    _abi.check(_abi.lib().gpk_line_clip(lines.handle, polys.handle, line_rows, poly_rows, n_rows, rows_space, mode, flags, out_src, src_space, stream, C.byref(h)))
    dev = DeviceGeoArray(h.value, GEOM_MULTILINESTRING, 0, -1)
    sizes = (C.c_int64 * 4)()
    _abi.check(_abi.lib().gpk_geoarray_download(dev.handle, sizes, None, None, None, None, stream))
    dev.n_coords, dev.n_geoms = int(sizes[0]), int(sizes[3])
    return GeoSeries(None, device=dev)


def take_args(op: str, a: GeoSeries, idx, allow_null: bool) -> np.ndarray:
    """the checks of take before any device call: a 1-D integer array whose every entry lies in [0, len) — or, with allow_null, is
    exactly -1.  Returns it as int64."""
    k = np.asarray(idx)
    if k.ndim != 1 or k.dtype.kind not in "iu":
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: `idx` must be a 1-D integer array (found {k.dtype}, {k.ndim}-D)")
    n = len(a)
    bad = (k >= n) | (k < (-1 if allow_null else 0)) if len(k) else np.zeros(0, bool)
    if bad.any():
        at = int(np.flatnonzero(bad)[0])
        raise _abi.GeopolarsHipError(
            _abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: idx[{at}] = {int(k[at])} is outside [0, {n})" + (" and is not -1" if allow_null else ""))
    return np.ascontiguousarray(k, dtype=np.int64)


def filter_args(op: str, a: GeoSeries, mask) -> np.ndarray:
    """the checks of filter before any device call: a 1-D bool array with one entry per row"""
    m = np.asarray(mask)
    if m.ndim != 1 or m.dtype != np.bool_:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: `mask` must be a 1-D bool array (found {m.dtype}, {m.ndim}-D)")
    if len(m) != len(a):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: {len(m)} mask entries for {len(a)} rows")
    return np.ascontiguousarray(m)


def segmentize_args(op: str, a: GeoSeries, max_segment_length):
    """the checks of segmentize before any device call: a real scalar > 0 (returned as a float), or a 1-D real array with one entry per
    row (returned as float64; its values are not looked at: NaN or <= 0 leaves a row unchanged)"""
    m = np.asarray(max_segment_length)
    if m.dtype.kind not in "iuf":
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: `max_segment_length` must be a number or an array of numbers (found {m.dtype})")
    if m.ndim == 0:
        if not float(m) > 0.0:
            raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: `max_segment_length` must be > 0 (found {float(m)})")
        return float(m)
    if m.ndim != 1 or len(m) != len(a):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"{op}: {m.shape} bounds for {len(a)} rows: one value per row")
    return np.ascontiguousarray(m, dtype=np.float64)


def polygon_clip_args(op: str, a: GeoSeries, b: GeoSeries, rows) -> Optional[np.ndarray]:
    """the checks of polygon_intersection / polygon_difference before any device call: polygons x polygons, then the row map as in
    intersection_measure_args"""
    return intersection_measure_args(op, POLYGONAL, a, b, rows)


def union_all_groups(a: GeoSeries, by) -> tuple[np.ndarray, int]:
    """the checks of union_all before any device call: a polygonal column, `by` None or a 1-D integer array with one entry per row.
    Returns (the rank of every row's group among the ascending distinct ids, the number of groups); None is one group."""
    if a._family() not in POLYGONAL:
        raise _mismatch(f"union_all: Polygon | MultiPolygon (found {_abi_name(a._family())})")
    if by is None:
        return np.zeros(len(a), dtype=np.int64), 1
    ids = np.asarray(by)
    if ids.dtype.kind not in "iu" or ids.ndim != 1:
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"union_all: `by` must be a 1-D integer array (found {ids.dtype}, {ids.ndim}-D)")
    if len(ids) != len(a):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"union_all: {len(ids)} group ids for {len(a)} rows")
    distinct, rank = np.unique(ids, return_inverse=True)
    return rank.astype(np.int64).reshape(-1), len(distinct)


def _union_all_live_rows(host: GeoArrowArray, groups: np.ndarray) -> np.ndarray:
    """the rows of a polygonal host column that are valid and have a coordinate, ordered by group (stable)"""
    g = host.geom_offsets.astype(np.int64)
    rings = g if host.geom_type == GEOM_POLYGON else host.part_offsets.astype(np.int64)[g]
    coords = host.ring_offsets.astype(np.int64)[rings]
    live = np.nonzero(host.is_valid() & (np.diff(coords) > 0))[0]
    return live[np.argsort(groups[live], kind="stable")]


def _as_multipolygon(host: GeoArrowArray) -> GeoArrowArray:
    """a POLYGON host column as a MULTIPOLYGON one of one member a row (offset surgery; a MULTIPOLYGON column is returned as it is)"""
    if host.geom_type != GEOM_POLYGON:
        return host
    return GeoArrowArray(_abi.GEOM_MULTIPOLYGON, host.xy, geom_offsets=np.arange(host.n_geoms + 1, dtype=np.int32), part_offsets=host.geom_offsets,
                         ring_offsets=host.ring_offsets, validity=host.validity, n_geoms=host.n_geoms)


def polygon_clip_call(a, b, a_rows, b_rows, n_rows: int, rows_space: int, mode: int, flags: int, out_src, src_space: int, out_status=None,
                      status_space: int = MEM_HOST, stream=None, entry: str = "gpk_polygon_clip") -> GeoSeries:
    """gpk_polygon_clip (or, as `entry`, gpk_polygon_union / gpk_polygon_symdiff, which take the same arguments) on two DeviceGeoArrays and raw row-list /
    output pointers: the owned MULTIPOLYGON result as a device-resident series"""
    h = C.c_void_p()
    _abi.check(getattr(_abi.lib(), entry)(a.handle, b.handle, a_rows, b_rows, n_rows, rows_space, mode, flags, out_src, src_space, out_status,
                                          status_space, stream, C.byref(h)))
    dev = DeviceGeoArray(h.value, _abi.GEOM_MULTIPOLYGON, 0, -1)
    sizes = (C.c_int64 * 4)()
    _abi.check(_abi.lib().gpk_geoarray_download(dev.handle, sizes, None, None, None, None, stream))
    dev.n_coords, dev.n_geoms = int(sizes[0]), int(sizes[3])
    return GeoSeries(None, device=dev)


def intersection_min_measure_arg(min_measure) -> float:
    """the `min_measure` of an intersection measure join as a float; anything but a finite number >= 0 is refused here, before any
    device call"""
    try:
        m = float(min_measure)
    except (TypeError, ValueError):
        m = float("nan")
    if not (m >= 0.0) or m == float("inf"):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"intersection measure join: min_measure must be a finite number >= 0, got {min_measure!r}")
    return m


def intersection_families_arg(op: str, left_family: int, right_family: int) -> None:
    """the family check of the intersection measure join, refused as the C ABI would: polygons or lines on the left, polygons on the
    right"""
    if (left_family in POLYGONAL or left_family in LINEAL) and right_family in POLYGONAL:
        return
    swap = ": the lines come first, swap the sides" if left_family in POLYGONAL and right_family in LINEAL else ""
    raise _mismatch(
        f"{op}: Polygon | MultiPolygon (area) or LineString | MultiLineString (length) x Polygon | MultiPolygon "
        f"(found {_abi_name(left_family)} x {_abi_name(right_family)}){swap}"
    )


def relation_sides(op: str, a: int, b: int) -> bool:
    """True when family `a` is lineal and `b` polygonal, False for the other order; any other pair is refused as the C ABI would"""
    if a in LINEAL and b in POLYGONAL:
        return True
    if a in POLYGONAL and b in LINEAL:
        return False
    raise _mismatch(f"{op}: LineString | MultiLineString x Polygon | MultiPolygon in either order (found {_abi_name(a)} x {_abi_name(b)})")


def relation_rows_arg(op: str, a: GeoSeries, b: GeoSeries, rows, line_first: bool) -> Optional[np.ndarray]:
    """the checks of line_polygon_relation before any device call: without a row map the row counts match; a row map (returned as
    uint32) has one entry per row of `a` and needs `a` to be the lineal side unless it is the identity"""
    return either_order_rows_arg(op, a, b, rows, line_first, "a row map needs the lineal column on the left (it maps line rows to polygon rows)")


FRECHET_MAX_SHORT = 16384  # GPK_FRECHET_MAX_SHORT of include/geopolars_hip.h
MAX_SUBDIVISIONS = 4096  # GPK_MAX_SUBDIVISIONS


def densify_arg(op: str, densify) -> int:
    """GeoPandas' densify fraction as the number of parts a segment is cut into: None -> 1, else round(1 / densify) (Python's round
    half to even, the rint of the JTS definition).  Anything but a finite number in (0, 1] whose count is at most MAX_SUBDIVISIONS is
    refused here with ValueError, before the library is called"""
    if densify is None:
        return 1
    try:
        f = float(densify)
    except (TypeError, ValueError):
        raise ValueError(f"{op}: densify must be None or a fraction in (0, 1], got {densify!r}") from None
    if isinstance(densify, (bool, np.bool_)) or not (0.0 < f <= 1.0):  # (NaN fails the comparison)
        raise ValueError(f"{op}: densify must be None or a fraction in (0, 1], got {densify!r}")
    k = 1.0 / f
    if not (k <= MAX_SUBDIVISIONS + 0.5) or round(k) > MAX_SUBDIVISIONS:
        raise ValueError(f"{op}: densify = {densify!r} cuts a segment into more than {MAX_SUBDIVISIONS} parts")
    return int(round(k))


def distance_rows_arg(op: str, a: GeoSeries, b: GeoSeries, rows) -> Optional[np.ndarray]:
    """the row pairing of hausdorff_distance / frechet_distance before any device call: without a row map the row counts match; a row
    map (returned as uint32) has one entry per row of `a`"""
    return paired_rows_arg(op, a, b, rows)


def dwithin_distance_arg(distance) -> float:
    """the `distance` of a dwithin call as a float; anything but a finite number >= 0 is refused here, before any device call"""
    try:
        d = float(distance)
    except (TypeError, ValueError):
        d = float("nan")
    if not (d >= 0.0) or d == float("inf"):
        raise _abi.GeopolarsHipError(_abi.GPK_ERR_INVALID_ARGUMENT, f"dwithin: distance must be a finite number >= 0, got {distance!r}")
    return d


class RowMap:
    """A row pairing (left row i -> right row rows[i]) ordered once for the grouped distance kernel (gpk_rowmap_build):
    reuse it for every batch of points that joins the same linestring column through the same foreign-key column."""

    def __init__(self, right: GeoSeries, rows, stream: int = 0):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        h = C.c_void_p()
        _abi.check(_abi.lib().gpk_rowmap_build(right.device().handle, rows.ctypes.data if len(rows) else None, len(rows), MEM_HOST, stream, C.byref(h)))
        self._h = h

    @staticmethod
    def from_device(right_dev: DeviceGeoArray, rows_tensor, stream: int = 0) -> "RowMap":
        """rows_tensor: int32/uint32 CUDA tensor (the map already in HBM)"""
        self = RowMap.__new__(RowMap)
        h = C.c_void_p()
        _abi.check(_abi.lib().gpk_rowmap_build(right_dev.handle, rows_tensor.data_ptr(), rows_tensor.shape[0], _abi.MEM_DEVICE, stream, C.byref(h)))
        self._h = h
        return self

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def free(self) -> None:
        if self._h:
            _abi.lib().gpk_rowmap_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _abi_name(t: int) -> str:
    from .geoarrow import GEOM_NAMES

    return GEOM_NAMES.get(t, f"type {t}")
