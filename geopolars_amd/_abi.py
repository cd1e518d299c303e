"""ctypes binding of include/geopolars_hip.h — the only door into libgeopolars_hip.so.

There is no CPU fallback behind this module: if the shared library is missing or a compute entry
point reports GPK_ERR_DEVICE, a GeopolarsHipError is raised.  `import torch` happens BEFORE the
library is opened so that libgeopolars_hip.so binds to the HIP runtime PyTorch already loaded
(same soname `libamdhip64.so.7`): device pointers from torch tensors and torch streams are then
valid inside the library, and torch.cuda.Event sees the library's launches.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPK_LIB_PATH") or os.path.join(HERE, "libgeopolars_hip.so")  # override: A/B builds

# ---- constants (mirror of the header) ----------------------------------------------------------
GPK_OK = 0
GPK_ERR_MISMATCHED_GEOMETRY = 1
GPK_ERR_INVALID_OFFSETS = 2
GPK_ERR_NULL_UNSUPPORTED = 3
GPK_ERR_DEVICE = 4
GPK_ERR_OOM = 5
GPK_ERR_INVALID_ARGUMENT = 6
GPK_ERR_CAPACITY = 7

GEOM_POINT = 0
GEOM_LINESTRING = 1
GEOM_POLYGON = 3
GEOM_MULTIPOINT = 4
GEOM_MULTILINESTRING = 5
GEOM_MULTIPOLYGON = 6
ARROW_WKB, ARROW_INTERLEAVED, ARROW_STRUCT = 0, 1, 2  # gpk_geoarray_to_arrow layouts

MEM_HOST = 0
MEM_DEVICE = 1

PRED_INTERSECTS = 0
PRED_CONTAINS = 1
PRED_WITHIN = 2
INDEX_BBOX_GRID = 1
INDEX_PIP = 2
INDEX_PIP_LIGHT = 4
INDEX_PIP_FULL = 8
QUERY_CONTAINED, QUERY_INTERSECTING = 0, 1  # gpk_index_query_envelope modes
PREDICATES = {"intersects": PRED_INTERSECTS, "contains": PRED_CONTAINS, "within": PRED_WITHIN}
LP_INTERIOR, LP_BOUNDARY, LP_EXTERIOR = 1, 2, 4  # GPK_LP_*: the bits of the line x polygon relation mask
LP_PRED_INTERSECTS, LP_PRED_WITHIN, LP_PRED_COVERED_BY, LP_PRED_CROSSES, LP_PRED_TOUCHES = 0, 1, 2, 3, 4  # GPK_LP_PRED_*
TRI_OK, TRI_EMPTY, TRI_FAILED = 0, 1, 2  # GPK_TRI_*: the row status of gpk_triangulate
CLIP_INSIDE, CLIP_OUTSIDE, CLIP_DROP_EMPTY = 0, 1, 1  # GPK_CLIP_*: the two modes of gpk_line_clip and its flag
PCLIP_INTERSECTION, PCLIP_DIFFERENCE = 0, 1  # GPK_PCLIP_*: the two modes of gpk_polygon_clip
PCLIP_OK, PCLIP_TOUCH, PCLIP_EMPTY, PCLIP_NULL, PCLIP_UNRESOLVED = 0, 1, 2, 3, 4  # the row status of gpk_polygon_clip
GEODESIC_AREA_SIGNED = 1  # GPK_GEODESIC_AREA_SIGNED
PUNION_UNION = 0  # GPK_PUNION_*: the mode of gpk_polygon_union (its row status is PCLIP_*)
PSYMDIFF_SYMMETRIC_DIFFERENCE = 0  # GPK_PSYMDIFF_*: the mode of gpk_polygon_symdiff (its row status is PCLIP_*)
PP_INTERIORS, PP_BOUNDARIES, PP_A_OUTSIDE, PP_B_OUTSIDE = 1, 2, 4, 8  # GPK_PP_*: the bits of the polygon x polygon relation mask
(PP_PRED_INTERSECTS, PP_PRED_WITHIN, PP_PRED_CONTAINS, PP_PRED_TOUCHES, PP_PRED_OVERLAPS, PP_PRED_EQUALS,
 PP_PRED_CONTAINS_PROPERLY) = range(7)  # GPK_PP_PRED_*
LL_INTERIORS, LL_SHARED_PIECE, LL_INT_BND, LL_BND_INT, LL_BND_BND, LL_A_OUTSIDE, LL_B_OUTSIDE = 1, 2, 4, 8, 16, 32, 64  # GPK_LL_*: the line x line mask
(LL_PRED_INTERSECTS, LL_PRED_WITHIN, LL_PRED_CONTAINS, LL_PRED_COVERED_BY, LL_PRED_COVERS, LL_PRED_CROSSES, LL_PRED_TOUCHES, LL_PRED_OVERLAPS,
 LL_PRED_EQUALS) = range(9)  # GPK_LL_PRED_*
PT_INTERIOR, PT_BOUNDARY, PT_EXTERIOR, PT_B_OUTSIDE = 1, 2, 4, 8  # GPK_PT_*: the bits of the point relation mask
GPK_KNN_MAX_K, GPK_KNN_EXCLUDE_SELF = 64, 1  # gpk_knn_join: the largest k, its one flag
(PT_PRED_INTERSECTS, PT_PRED_WITHIN, PT_PRED_CONTAINS, PT_PRED_COVERED_BY, PT_PRED_COVERS, PT_PRED_CROSSES, PT_PRED_TOUCHES, PT_PRED_OVERLAPS,
 PT_PRED_EQUALS) = range(9)  # GPK_PT_PRED_*


class GeopolarsHipError(RuntimeError):
    """Mirror of GeopolarsError (geopolars/geopolars-geo/src/error.rs:9-28) on the Python side."""

    def __init__(self, code: int, message: str):
        super().__init__(f"[gpk status {code}] {message}")
        self.code = code


class MismatchedGeometry(GeopolarsHipError):
    """GeopolarsError::MismatchedGeometry (error.rs:12-16)."""


class GeoArrowDesc(C.Structure):
    _fields_ = [
        ("geom_type", C.c_int32),
        ("mem_space", C.c_int32),
        ("n_geoms", C.c_int64),
        ("n_coords", C.c_int64),
        ("xy", C.c_void_p),
        ("geom_offsets", C.c_void_p),
        ("part_offsets", C.c_void_p),
        ("ring_offsets", C.c_void_p),
        ("n_parts", C.c_int64),
        ("n_rings", C.c_int64),
        ("validity", C.c_void_p),
        ("x", C.c_void_p),  # separated coordinates (xy NULL): Struct<x, y> GeoArrow arrays
        ("y", C.c_void_p),
    ]


class ArrowSchema(C.Structure):
    """Arrow C Data Interface (what `pyarrow.Array._export_to_c` fills: py-geopolars/src/ffi.rs:12-32)"""


ArrowSchema._fields_ = [
    ("format", C.c_char_p),
    ("name", C.c_char_p),
    ("metadata", C.c_void_p),
    ("flags", C.c_int64),
    ("n_children", C.c_int64),
    ("children", C.POINTER(C.POINTER(ArrowSchema))),
    ("dictionary", C.POINTER(ArrowSchema)),
    ("release", C.CFUNCTYPE(None, C.POINTER(ArrowSchema))),
    ("private_data", C.c_void_p),
]


class ArrowArray(C.Structure):
    pass


ArrowArray._fields_ = [
    ("length", C.c_int64),
    ("null_count", C.c_int64),
    ("offset", C.c_int64),
    ("n_buffers", C.c_int64),
    ("n_children", C.c_int64),
    ("buffers", C.POINTER(C.c_void_p)),
    ("children", C.POINTER(C.POINTER(ArrowArray))),
    ("dictionary", C.POINTER(ArrowArray)),
    ("release", C.CFUNCTYPE(None, C.POINTER(ArrowArray))),
    ("private_data", C.c_void_p),
]


# every symbol the header declares: name -> (restype, argtypes)
_VP = C.c_void_p
_PROTOS = {
    "gpk_version": (C.c_char_p, []),
    "gpk_last_error": (C.c_int32, [C.c_char_p, C.c_size_t]),
    "gpk_device_count": (C.c_int32, [C.POINTER(C.c_int32)]),
    "gpk_device_info": (C.c_int32, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]),
    "gpk_geoarray_upload": (C.c_int32, [C.POINTER(GeoArrowDesc), _VP, C.POINTER(_VP)]),
    "gpk_geoarray_from_arrow": (C.c_int32, [_VP, _VP, C.c_int32, _VP, C.POINTER(_VP), C.POINTER(C.c_int32)]),
    "gpk_geoarray_to_arrow": (C.c_int32, [_VP, C.c_int32, _VP, _VP, _VP]),
    "gpk_geoarray_free": (C.c_int32, [_VP]),
    "gpk_geoarray_invalidate": (C.c_int32, [_VP]),
    "gpk_geoarray_nbytes": (C.c_int32, [_VP, C.POINTER(C.c_int64)]),
    "gpk_wkb_decode": (C.c_int32, [_VP, _VP, C.c_int64, _VP, C.POINTER(C.c_int64), _VP, _VP, _VP, _VP]),
    "gpk_geoarray_from_wkb": (C.c_int32, [_VP, _VP, C.c_int64, _VP, C.c_int32, _VP, C.POINTER(_VP), C.POINTER(C.c_int32)]),
    "gpk_geoarray_download": (C.c_int32, [_VP, C.POINTER(C.c_int64), _VP, _VP, _VP, _VP, _VP]),
    "gpk_area": (C.c_int32, [_VP, _VP, C.c_int32, _VP]),
    "gpk_signed_area": (C.c_int32, [_VP, _VP, C.c_int32, _VP]),
    "gpk_centroid": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_representative_point": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_bounds": (C.c_int32, [_VP, _VP, C.c_int32, _VP]),
    "gpk_euclidean_length": (C.c_int32, [_VP, _VP, C.c_int32, _VP]),
    "gpk_affine_transform": (C.c_int32, [_VP, C.POINTER(C.c_double), _VP, C.c_int32, _VP]),
    "gpk_affine_transform_rows": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_affine_about_origin": (C.c_int32, [_VP, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double, _VP, C.c_int32, _VP]),
    "gpk_crs_supported": (C.c_int32, [C.c_int32]),
    "gpk_reproject": (C.c_int32, [_VP, C.c_int32, C.c_int32, _VP, C.POINTER(C.c_int64), C.c_int32, _VP]),
    "gpk_envelope": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_exterior": (C.c_int32, [_VP, _VP, _VP, C.POINTER(C.c_int64), C.c_int32, _VP]),
    "gpk_explode": (C.c_int32, [_VP, _VP, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_geoarray_validity": (C.c_int32, [_VP, _VP, C.POINTER(C.c_int32), _VP]),
    "gpk_geoarray_len": (C.c_int32, [_VP, C.POINTER(C.c_int64)]),
    "gpk_geom_type": (C.c_int32, [_VP, _VP, C.c_int32, _VP]),
    "gpk_is_empty": (C.c_int32, [_VP, _VP, C.c_int32, _VP]),
    "gpk_is_ring": (C.c_int32, [_VP, _VP, C.c_int32, _VP]),
    "gpk_point_xy": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_geodesic_length": (C.c_int32, [_VP, C.c_int32, _VP, C.c_int32, _VP]),
    "gpk_geodesic_area": (C.c_int32, [_VP, C.c_uint32, _VP, _VP, C.c_int32, _VP]),
    "gpk_geodesic_inverse": (C.c_int32, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_geodesic_direct": (C.c_int32, [_VP, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP, C.c_int32, _VP]),
    "gpk_simplify": (C.c_int32, [_VP, C.c_double, _VP, _VP, C.POINTER(C.c_int64), C.c_int32, _VP]),
    "gpk_convex_hull": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_minimum_rotated_rectangle": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_minimum_bounding_circle": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_distance_rowwise": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_rowmap_build": (C.c_int32, [_VP, _VP, C.c_int64, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_rowmap_free": (C.c_int32, [_VP]),
    "gpk_rowmap_nbytes": (C.c_int32, [_VP, C.POINTER(C.c_int64)]),
    "gpk_distance_rowmap": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_hausdorff_distance": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP, C.c_int32, _VP]),
    "gpk_frechet_distance": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP, C.POINTER(C.c_int64), C.c_int32, _VP]),
    "gpk_predicate_rowwise": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP, C.c_int32, _VP]),
    "gpk_index_build": (C.c_int32, [_VP, _VP, C.POINTER(_VP)]),
    "gpk_index_build_ex": (C.c_int32, [_VP, C.c_int32, _VP, _VP, C.POINTER(_VP)]),
    "gpk_index_free": (C.c_int32, [_VP]),
    "gpk_index_nbytes": (C.c_int32, [_VP, C.POINTER(C.c_int64)]),
    "gpk_index_describe": (C.c_int32, [_VP, C.POINTER(C.c_int64)]),
    "gpk_index_query_envelope": (C.c_int32, [_VP, _VP, C.c_int64, C.c_int32, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP]),
    "gpk_spatial_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_int32, C.c_uint32, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_spatial_join_async": (C.c_int32, [_VP, _VP, _VP, C.c_int32, C.c_uint32, _VP, _VP, C.c_int64, _VP, _VP]),
    "gpk_nearest_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_double, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_nearest_join_any": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_double, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_knn_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_int32, C.c_double, C.c_uint32, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_dwithin_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_double, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_dwithin_rowwise": (C.c_int32, [_VP, _VP, _VP, C.c_double, _VP, C.c_int32, _VP]),
    "gpk_line_polygon_relation": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_line_polygon_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_int32, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_polygon_relation": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_polygon_relation_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_int32, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_intersection_measure": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_line_clip": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_polygon_clip": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, C.c_int32, _VP, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_polygon_union": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, C.c_int32, _VP, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_polygon_symdiff": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, C.c_int32, _VP, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_union_all_pairs": (C.c_int32, [_VP, _VP, C.c_int64, C.c_int64, _VP, _VP, _VP, _VP, C.POINTER(C.c_int64), _VP]),
    "gpk_intersection_measure_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_double, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_line_relation": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_line_relation_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_int32, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_point_relation": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_point_relation_join": (
        C.c_int32,
        [_VP, _VP, _VP, C.c_int32, C.c_uint32, _VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP],
    ),
    "gpk_validity": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_is_simple": (C.c_int32, [_VP, _VP, C.c_int32, _VP]),
    "gpk_triangulate": (C.c_int32, [_VP, _VP, C.c_int64, _VP, _VP, C.POINTER(C.c_int64), C.c_int32, _VP]),
    "gpk_closest_point_rowwise": (C.c_int32, [_VP, _VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gpk_line_locate_point": (C.c_int32, [_VP, _VP, _VP, C.c_int32, _VP, C.c_int32, _VP]),
    "gpk_line_interpolate_point": (C.c_int32, [_VP, _VP, C.c_int64, C.c_int32, _VP, _VP, C.c_int32, _VP]),
    "gpk_wkb_encode": (C.c_int32, [_VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64)]),
    "gpk_geoarray_to_wkb": (C.c_int32, [_VP, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP]),
    "gpk_join_indices": (C.c_int32, [_VP, _VP, C.c_int64, C.c_int64, C.c_uint32, C.c_int32, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _VP]),
    "gpk_take_fixed": (C.c_int32, [_VP, C.c_int32, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP, C.c_int32, _VP]),
    "gpk_take_binary": (C.c_int32, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP, C.c_int64, C.POINTER(C.c_int64), _VP, C.c_int32, _VP]),
    "gpk_geoarray_take": (C.c_int32, [_VP, _VP, C.c_int64, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_geoarray_filter": (C.c_int32, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.POINTER(_VP), C.POINTER(C.c_int64)]),
    "gpk_segmentize": (C.c_int32, [_VP, C.c_double, _VP, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_remove_repeated_points": (C.c_int32, [_VP, C.c_double, _VP, C.POINTER(_VP)]),
    "gpk_reverse": (C.c_int32, [_VP, _VP, C.POINTER(_VP)]),
    "gpk_orient_polygons": (C.c_int32, [_VP, C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_comm_unique_id":(C.c_int32, [C.POINTER(C.c_uint8)]),
    "gpk_comm_init": (C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(_VP)]),
    "gpk_comm_free": (C.c_int32, [_VP]),
    "gpk_comm_mock_world": (C.c_int32, [C.c_int32, C.POINTER(_VP)]),
    "gpk_comm_init_mock": (C.c_int32, [C.c_int32, _VP, C.POINTER(_VP)]),
    "gpk_comm_mock_world_free": (C.c_int32, [_VP]),
    "gpk_comm_info": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gpk_allgatherv_geoarray": (C.c_int32, [_VP, _VP, _VP, C.POINTER(_VP), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gpk_geoarray_concat": (C.c_int32, [C.POINTER(_VP), C.c_int32, _VP, C.POINTER(_VP), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gpk_allgatherv_rows_f64": (C.c_int32, [_VP, _VP, C.c_int64, C.c_int32, _VP, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _VP]),
    "gpk_device_cache_release": (C.c_int32, []),
    "gpk_join_stats_enable": (C.c_int32, [C.c_int32]),
    "gpk_join_stats": (C.c_int32, [C.POINTER(C.c_int64), C.c_int32]),
    "gpk_profile_enable": (C.c_int32, [C.c_int32]),
    "gpk_profile_filter": (C.c_int32, [C.c_char_p]),
    "gpk_profile_reset": (C.c_int32, []),
    "gpk_profile_query": (C.c_int32, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)

_lib = None


def lib() -> C.CDLL:
    """Open libgeopolars_hip.so (once).  Fails loudly when the HIP extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GeopolarsHipError(
            GPK_ERR_DEVICE,
            f"{LIB_PATH} is missing: build it with `python -m geopolars_amd.build` "
            "(hipcc, gfx950).  geopolars_amd has no CPU fallback.",
        )
    try:  # make the process-wide HIP runtime the one torch ships, before our DT_NEEDED is resolved
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing, the C ABI works without it
        pass
    handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(handle, name)  # AttributeError here == header/library drift
        fn.restype = res
        fn.argtypes = args
    _lib = handle
    return _lib


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib().gpk_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(status: int) -> None:
    if status == GPK_OK:
        return
    msg = last_error()
    if status == GPK_ERR_MISMATCHED_GEOMETRY:
        raise MismatchedGeometry(status, msg)
    raise GeopolarsHipError(status, msg)


def device_count() -> int:
    n = C.c_int32(0)
    rc = lib().gpk_device_count(C.byref(n))
    return int(n.value) if rc == GPK_OK else 0


def device_info() -> tuple[str, int]:
    buf = C.create_string_buffer(256)
    cus = C.c_int32(0)
    check(lib().gpk_device_info(buf, 256, C.byref(cus)))
    return buf.value.decode(), int(cus.value)
