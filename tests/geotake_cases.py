"""Columns, index lists and the expected result shared by tests/test_geotake_host.py and tests/test_gpu_geotake.py.

The expected value everywhere is GeoArrowArray.take on the host.  An index outside [0, n) is added by hand: the column gets one more
row — null, without children, (NaN, NaN) in a POINT column — and such an index reads that row.

The fill of csrc/gpk_geotake.hip works on strips of STRIP = 1024 output elements (coordinates, or entries of an offsets level) and
stages at most WINDOW = 2048 row starts of a strip in LDS; the hand-built columns below sit on those two numbers."""
import numpy as np

from geopolars_amd import _abi, synth
from geopolars_amd.geoarrow import GeoArrowArray
from tests.second_pass import same_bits

STRIP, WINDOW = 1024, 2048


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    return off


def _xy(n, seed):
    return np.random.default_rng(seed).uniform(-100, 100, (n, 2))


def multipoints(n, seed):
    rng = np.random.default_rng(seed)
    off = _offsets(rng.integers(0, 5, n))
    return GeoArrowArray(_abi.GEOM_MULTIPOINT, rng.uniform(0, 100, (int(off[-1]), 2)), geom_offsets=off)


def multilinestrings(n, seed):
    rng = np.random.default_rng(seed)
    go = _offsets(rng.integers(0, 4, n))
    ro = _offsets(rng.integers(2, 7, int(go[-1])))
    return GeoArrowArray(_abi.GEOM_MULTILINESTRING, rng.uniform(0, 100, (int(ro[-1]), 2)), geom_offsets=go, ring_offsets=ro)


def with_nulls(a: GeoArrowArray, seed: int, p: float = 0.2) -> GeoArrowArray:
    """the same column with a validity bitmap: the children of its null rows stay where they are"""
    valid = np.random.default_rng(seed).uniform(size=len(a)) > p
    return GeoArrowArray(a.geom_type, a.xy, a.geom_offsets, a.part_offsets, a.ring_offsets, np.packbits(valid, bitorder="little"), n_geoms=len(a))


def columns():
    """the six types (hundreds of rows, as tests/test_gpu_concat.py::_columns), one with nulls, plus a POINT column with nulls; the
    coordinates carry NaN payloads and signed zeros"""
    pts = synth.uniform_points(1003, seed=2)
    poly = synth.clustered_polygons(701, seed=4)
    poly.xy[::7, 0] = -0.0
    poly.xy[5::11].view(np.uint64)[:, 1] = 0x7FF8_0000_DEAD_BEEF  # a NaN with a payload
    poly.xy[3::13].view(np.uint64)[:, 0] = 0xFFF0_0000_0000_0001  # a signalling one, sign set
    return {
        "point": pts,
        "point+nulls": with_nulls(pts, 11),
        "linestring": synth.random_linestrings(517, seed=3),
        "polygon": poly,
        "multipoint": multipoints(333, 5),
        "multilinestring": multilinestrings(411, 6),
        "multipolygon": synth.powerlaw_multipolygons(257, seed=7),
        "multipolygon+nulls": with_nulls(synth.powerlaw_multipolygons(129, seed=8), 12),
    }


def edge_columns():
    """the smallest shapes at which the fill can go wrong (STRIP = 1024 output elements, WINDOW = 2048 staged row starts)"""
    out = {}
    # a row of 2500 coordinates spans three strips; the next rows end exactly on a strip boundary (3072), one before the next (4095)
    # and one after it (4097)
    lens = [2500, 572, 1023, 2, 7, 1017, 1, 1024, 3]
    out["linestring strips"] = GeoArrowArray(_abi.GEOM_LINESTRING, _xy(sum(lens), 21), geom_offsets=_offsets(lens))
    # 5000 one-coordinate rows: 1024 rows a strip
    out["multipoint 5000 x 1"] = GeoArrowArray(_abi.GEOM_MULTIPOINT, _xy(5000, 22), geom_offsets=_offsets([1] * 5000))
    # 5000 consecutive empty rows between two non-empty ones: more row starts in one strip than the window holds
    lens = [3] + [0] * 5000 + [4] + [0] * 3 + [2]
    out["multipoint empty run"] = GeoArrowArray(_abi.GEOM_MULTIPOINT, _xy(sum(lens), 23), geom_offsets=_offsets(lens))
    # the same through an offsets level: polygons without rings, a ring without coordinates
    rings = [2] + [0] * 5000 + [1, 0, 3]
    rlens = [5, 4] + [6] + [4, 0, 5]
    out["polygon empty run"] = GeoArrowArray(_abi.GEOM_POLYGON, _xy(sum(rlens), 24), geom_offsets=_offsets(rings), ring_offsets=_offsets(rlens))
    # a MULTIPOLYGON whose rows have zero parts, parts without rings, rings without coordinates
    parts = [0, 2, 0, 0, 1, 3, 0]
    prings = [1, 2, 0, 1, 0, 2]
    rlens = [4, 5, 4, 7, 0, 4]
    out["multipolygon zero parts"] = GeoArrowArray(_abi.GEOM_MULTIPOLYGON, _xy(sum(rlens), 25), geom_offsets=_offsets(parts),
                                                   part_offsets=_offsets(prings), ring_offsets=_offsets(rlens))
    # a column whose every row is empty: the result's coordinate total is 0
    out["multilinestring all empty"] = GeoArrowArray(_abi.GEOM_MULTILINESTRING, np.zeros((0, 2)), geom_offsets=_offsets([0, 2, 0, 1]),
                                                     ring_offsets=_offsets([0, 0, 0]))
    return out


def index_lists(n, seed=0):
    """{name: int64 indices into a column of n rows}"""
    rng = np.random.default_rng(seed)
    mixed = rng.integers(0, max(n, 1), 3 * 8 + 5).astype(np.int64)
    mixed[::4] = -1
    mixed[1::6] = n
    assert len(mixed) % 8 != 0
    return {
        "identity": np.arange(n, dtype=np.int64),
        "reverse": np.arange(n, dtype=np.int64)[::-1].copy(),
        "permutation": rng.permutation(n).astype(np.int64),
        "3n draws": rng.integers(0, max(n, 1), 3 * n).astype(np.int64),
        "sorted repeats": np.sort(rng.integers(0, max(n, 1), n + 3)).astype(np.int64),
        "empty": np.zeros(0, np.int64),
        "single": np.array([n // 2], np.int64),
        "all -1": np.full(13, -1, np.int64),
        "mixed -1 and n": mixed,
    }


def expected_take(host: GeoArrowArray, idx) -> GeoArrowArray:
    """GeoArrowArray.take, with an index outside [0, n) reading a null row without children ((NaN, NaN) in a POINT column)"""
    idx = np.asarray(idx, dtype=np.int64)
    n = len(host)
    bad = (idx < 0) | (idx >= n)
    if not bad.any():
        return host.take(idx)
    valid = np.packbits(np.concatenate([host.is_valid(), [False]]).astype(np.uint8), bitorder="little")
    if host.geom_type == _abi.GEOM_POINT:
        more = GeoArrowArray(_abi.GEOM_POINT, np.concatenate([host.xy, [[np.nan, np.nan]]]), validity=valid)
    else:
        more = GeoArrowArray(host.geom_type, host.xy, np.concatenate([host.geom_offsets, host.geom_offsets[-1:]]), host.part_offsets,
                             host.ring_offsets, valid, n_geoms=n + 1)
    return more.take(np.where(bad, n, idx))


def assert_same(got: GeoArrowArray, want: GeoArrowArray, what=""):
    """level by level, is_valid(), the coordinates bit for bit, and whether there is a bitmap at all"""
    assert got.geom_type == want.geom_type and len(got) == len(want), what
    for name in ("geom_offsets", "part_offsets", "ring_offsets"):
        x, y = getattr(got, name), getattr(want, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert np.array_equal(x, y), (what, name)
    assert same_bits(got.xy, want.xy), (what, "xy")
    assert np.array_equal(got.is_valid(), want.is_valid()), (what, "validity")
    assert (got.validity is None) == (want.validity is None), (what, "has a bitmap")
