"""Point relations, host side: the per-pair routine of csrc/gpk_pointrel.h run on the CPU at G = 1 by a stand-alone program — plain and
under AddressSanitizer + UBSan — against tests/pointrel_ref.py, mask for mask; and the checks that need no device: the C ABI symbols,
the header's bits, ids and mapping, the refusals that come before any device work, the transposition of names, the routers' dispatch
table, and the older methods that must keep refusing."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import (
    LINE_MASK_PREDICATES,
    MASK_PREDICATES,
    POINT_MASK_PREDICATES,
    POLYGON_MASK_PREDICATES,
    GeoSeries,
    family_dim,
    point_mask_predicate,
    point_relation_rows_arg,
    point_transposed,
    predicate_route,
)
from geopolars_amd.spatial_index import (
    POINT_RELATION_PREDICATES,
    SJOIN_ROUTES,
    SpatialJoinRelationArgs,
    line_relation_pairs,
    point_relation_pairs,
    point_relation_pairs_device,
    point_relation_predicate_arg,
    polygon_relation_pairs,
    relation_pairs,
    sjoin,
    sjoin_pairs,
    spatial_join_point_relation,
)
from tests import pointrel_ref as P
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PT, MPT, LS, MLS, PG, MPG = P.PT, P.MPT, P.LS, P.MLS, P.PG, P.MPG
FAMILY_IDS = [f"{P.NAMES[a]}-{P.NAMES[b]}" for a, b in P.FAMILIES]
BUILDS = ["plain", "sanitized"]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "pointrel", fp_contract_off=False)


def _record(ka, row_a, kb, row_b) -> bytes:
    pa = P._coords(ka, row_a)
    d = P.DIM[kb]
    if d == 0:
        seqs, pb = None, P._coords(kb, row_b)
    else:
        seqs = [list(s) for s in (P.L.members(kb, row_b) if d == 1 else [r for g in ([row_b] if kb == PG else row_b) for r in g])]
        pb = [p for s in seqs for p in s]
    out = struct.pack("<iiiii", int(ka == PT), d, len(pa), 0 if seqs is None else len(seqs), len(pb))
    out += np.asarray(pa, dtype="<f8").reshape(-1, 2).tobytes()
    if seqs:
        out += np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype("<i4").tobytes()
    return out + np.asarray(pb, dtype="<f8").reshape(-1, 2).tobytes()


def _run(exe, workdir, ka, rows_a, kb, rows_b):
    """-> (masks, predicates[n, 9] computed with each predicate's early stop)"""
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    with open(fin, "wb") as f:
        for ra, rb in zip(rows_a, rows_b):
            f.write(_record(ka, ra, kb, rb))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.uint8).reshape(len(rows_a), 10)
    return raw[:, 0], raw[:, 1:].astype(bool)


def _check(built, workdir, build, ka, rows_a, kb, rows_b, want, what):
    got, preds = _run(built[build], workdir, ka, rows_a, kb, rows_b)
    assert np.array_equal(got, want), (what, [(i, int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])
    for name, pid in P.PRED_IDS.items():
        exp = np.array([P.PREDICATES[name](int(m), P.DIM[kb]) for m in want])
        assert np.array_equal(preds[:, pid], exp), (what, name)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_driver_matches_the_reference(drivers, build, ka, kb):
    """KNOWN and TIES as they are and padded, and the random columns: the full mask, and every predicate from the mask its own early
    stop leaves"""
    built, workdir = drivers
    for cases in (P.KNOWN, P.TIES):
        for pad in (0, 7):
            a, b, want, _ = P.case_columns(cases, ka, kb, pad)
            if len(a):
                _check(built, workdir, build, ka, a, kb, b, want, (pad, "cases"))
    A, B, want = P.random_columns(ka, kb)
    assert P.honest(ka, kb, want)
    _check(built, workdir, build, ka, A, kb, B, want, "random")


@pytest.mark.parametrize("build", BUILDS)
def test_driver_on_unusable_rows_and_large_rows(drivers, build):
    built, workdir = drivers
    sq = P.SQ4[0]
    rows_b = [[sq], [sq[:-1]], [sq[:2] + sq[:1]], [[(0, 0), (2, 2), (4, 4), (0, 0)]], [sq, []], [[]], []]
    want = np.array([9, 0, 0, 0, 9, 0, 0], dtype=np.uint8)  # unclosed, 3 coordinates, collinear: unusable; an empty hole is ignored
    got, _ = _run(built[build], workdir, PT, [(1, 1)] * len(rows_b), PG, rows_b)
    assert np.array_equal(got, want)
    assert np.array_equal(P.masks(PT, [(1, 1)] * len(rows_b), PG, rows_b), want)
    got, _ = _run(built[build], workdir, MPT, [[], [(1, 1)]], MLS, [[[(0, 0), (2, 2)]], [[], []]])
    assert not got.any()
    pts = [(x, y) for x in range(0, 40, 3) for y in range(-2, 6)]
    for kb, row in ((LS, P.zigzag()), (PG, P.big_donut())):
        got, _ = _run(built[build], workdir, MPT, [pts], kb, [row])
        assert got[0] == P.mask(MPT, pts, kb, row) and got[0] & 7 == 7  # points inside, on the boundary and outside


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
NAMES = ("gpk_point_relation", "gpk_point_relation_join")


def test_exported_symbols_name_the_point_relation_calls():
    for name in NAMES:
        assert name in _abi.EXPORTED_SYMBOLS
    assert _abi._PROTOS["gpk_point_relation"] == _abi._PROTOS["gpk_line_relation"]
    assert _abi._PROTOS["gpk_point_relation_join"] == _abi._PROTOS["gpk_line_relation_join"]
    assert (_abi.PT_INTERIOR, _abi.PT_BOUNDARY, _abi.PT_EXTERIOR, _abi.PT_B_OUTSIDE) == (1, 2, 4, 8)


def test_built_library_exports_the_calls():
    from geopolars_amd import build

    names = exported_symbols()
    assert set(NAMES) <= names
    assert "gpk_pointrel.hip" in build.SOURCES


def test_headers_state_the_bits_ids_and_the_mapping():
    text = open(os.path.join(ROOT, "include", "geopolars_hip.h")).read()
    defs = dict(re.findall(r"#define (GPK_PT_\w+) (\d+)", text))
    assert defs == {"GPK_PT_INTERIOR": "1", "GPK_PT_BOUNDARY": "2", "GPK_PT_EXTERIOR": "4", "GPK_PT_B_OUTSIDE": "8",
                    **{f"GPK_PT_PRED_{n.upper()}": str(i) for n, i in P.PRED_IDS.items()}}
    assert {n: getattr(_abi, f"PT_PRED_{n.upper()}") for n in P.PRED_IDS} == P.PRED_IDS == POINT_RELATION_PREDICATES
    assert P.PRED_IDS == P.L.PRED_IDS  # numbered as GPK_LL_PRED_*
    flat = " ".join(text.replace(" * ", " ").split())
    for line in ("intersects mask & 3", "disjoint mask != 0 && !(mask & 3)", "within (mask & 1) && !(mask & 4)", "covered_by (mask & 3) && !(mask & 4)",
                 "contains (mask & 1) && !(mask & 8)", "covers (mask & 3) && !(mask & 8)", "touches (mask & 2) && !(mask & 1)",
                 "equals (mask & 1) && !(mask & 12)", "crosses dim(B) >= 1: (mask & 1) && (mask & 4); dim(B) == 0: never",
                 "overlaps dim(B) == 0: (mask & 13) == 13; dim(B) >= 1: never", "II, IB, IE are the bits 1, 2, 4", "with the bits 4 and 8 swapped",
                 "1, 5, 9, 12, 13 for a punctual B, 9 .. 15 for a polygonal B"):
        assert line in flat, line
    rule = open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_pointrel.h")).read()
    for line in ("II, IB, IE are the bits 1, 2, 4", "bit 8 is \"EI or EB non-empty\"", "with the bits 4 and 8 swapped", "punctual B     1, 5, 9, 12, 13",
                 "polygonal B    9 .. 15", "degenerate additionally 1, 5", "constexpr int64_t PT_LARGE_COST = PD_LARGE_COST;  // a first value, not swept"):
        assert line in rule, line
    for fn in ("gpk_pointrel.h", "gpk_pointrel.hip"):  # uncapped grids: nothing for tests/second_pass.py to list
        assert not re.search(r"\bcu_count\(\)|\bgroup_grid\(", open(os.path.join(ROOT, "geopolars_amd", "csrc", fn)).read()), fn


def test_mask_to_predicate_table_for_all_16_masks():
    masks = np.arange(16, dtype=np.uint8)
    assert set(POINT_MASK_PREDICATES) == set(P.PREDICATES) | {"contains_properly"}
    for d in (0, 1, 2):
        for name, f in P.PREDICATES.items():
            got = point_mask_predicate(masks, name, d)
            assert got.dtype == bool and got.tolist() == [f(int(m), d) for m in masks], (name, d)
        assert np.array_equal(point_mask_predicate(masks, "contains_properly", d), point_mask_predicate(masks, "contains", d))
        assert not any(point_mask_predicate(np.zeros(1, dtype=np.uint8), n, d)[0] for n in POINT_MASK_PREDICATES)
    for name, d in (("dwithin", 0), ("within", 3)):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            point_mask_predicate(masks, name, d)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_names_are_transposed_for_a_punctual_column_on_the_right():
    assert [point_transposed(n) for n in ("within", "contains", "covered_by", "covers")] == ["contains", "within", "covers", "covered_by"]
    for n in ("intersects", "disjoint", "touches", "equals", "crosses", "overlaps"):
        assert point_transposed(n) == n
    # B contains A properly: every point of A in B's interior
    masks = np.arange(16, dtype=np.uint8)
    assert point_mask_predicate(masks, point_transposed("contains_properly"), 2).tolist() == [(m & 7) == 1 for m in range(16)]
    assert {n: P.TRANSPOSED.get(n, n) for n in P.PRED_IDS} == {n: point_transposed(n) for n in P.PRED_IDS}


def test_the_routers_dispatch_table():
    kinds = (PT, MPT, LS, MLS, PG, MPG)
    assert [family_dim(k) for k in kinds] == [0, 0, 1, 1, 2, 2]
    for a in kinds:
        for b in kinds:
            route, names = predicate_route(a, b)
            da, db = family_dim(a), family_dim(b)
            want = "point" if 0 in (da, db) else {(1, 1): "line", (2, 2): "polygon"}.get((da, db), "line_polygon")
            assert route == want, (a, b)
            assert names is {"point": POINT_MASK_PREDICATES, "line": LINE_MASK_PREDICATES, "polygon": POLYGON_MASK_PREDICATES, "line_polygon": MASK_PREDICATES}[route]
    assert {k: v[1] for k, v in SJOIN_ROUTES.items()} == {"point": point_relation_pairs, "line": line_relation_pairs, "polygon": polygon_relation_pairs,
                                                           "line_polygon": relation_pairs}
    for bad in (2, 7, -1):  # GEOMETRYCOLLECTION and unknown codes: an explicit error
        with pytest.raises(_abi.MismatchedGeometry):
            predicate_route(bad, PT)
        with pytest.raises(_abi.MismatchedGeometry):
            predicate_route(PG, bad)


def test_bad_arguments_are_refused_by_the_library_before_any_device_work():
    """a NULL column, output or count; an unknown predicate id (checked first, before a handle is read: 64 stands in for one)"""
    lib = _abi.lib()
    fake = C.c_void_p(64)
    out = np.zeros(4, dtype=np.uint8)
    n = C.c_int64(-1)
    for a, b, o in ((None, fake, out.ctypes.data), (fake, None, out.ctypes.data), (fake, fake, None)):
        assert lib.gpk_point_relation(a, b, None, o, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    for a, b, np_ in ((None, fake, C.byref(n)), (fake, None, C.byref(n)), (fake, fake, None)):
        assert lib.gpk_point_relation_join(a, b, None, 0, 0, None, None, None, 0, np_, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    for pred in (-1, 9, 99):
        assert lib.gpk_point_relation_join(fake, fake, None, pred, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
        assert "point_relation_join: unknown predicate" in _abi.last_error() and n.value == 0
    assert not out.any()


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]))
    two = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]))
    line = [(0.0, 0.0), (1.0, 1.0)]
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    return pts, two, GeoSeries(GeoArrowArray.from_linestrings([line] * 3)), GeoSeries(GeoArrowArray.from_polygons([sq] * 3))


def test_argument_errors_come_before_the_device(no_device):
    pts, two, lines, polys = _series()
    for call in (lambda: lines.point_relation(polys), lambda: polys.point_relation(polys), lambda: lines.point_relation(lines),
                 lambda: lines.point_predicate(polys, "touches"), lambda: point_relation_pairs(lines, polys), lambda: point_relation_pairs(polys, polys, "touches"),
                 lambda: point_relation_pairs_device(lines, lines, None, "touches", None, None)):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    for call in (
        lambda: pts.point_relation(two),  # 3 rows against 2
        lambda: pts.point_relation(two, other_rows=[0, 1]),  # one entry per row of self
        lambda: pts.point_relation(two, other_rows=[[0, 1, 0]]),
        lambda: pts.point_relation(two, other_rows=["a", "b", "c"]),
        lambda: lines.point_relation(pts, other_rows=[2, 1, 0]),  # a row map needs the punctual side in self
        lambda: pts.point_predicate(lines, "dwithin"),
        lambda: lines.point_predicate(polys, "dwithin"),  # the name before the families
        lambda: pts.predicate(lines, "dwithin"),
        lambda: lines.predicate(lines, "contains_properly"),  # the line relations have no such name
        lambda: lines.predicate(polys, "overlaps"),
        lambda: point_relation_pairs(pts, lines, "disjoint"),
        lambda: point_relation_pairs(lines, polys, "disjoint"),  # the predicate before the families
        lambda: point_relation_pairs_device(pts, two, None, "dwithin", None, None),
        lambda: sjoin_pairs(pts, lines, "contains_properly"),
        lambda: sjoin_pairs(lines, polys, "overlaps"),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT and not isinstance(e.value, _abi.MismatchedGeometry)
    assert point_relation_rows_arg("point_relation", pts, two, [1, 0, 7], True).dtype == np.uint32
    assert point_relation_rows_arg("point_relation", pts, pts, None, True) is None
    assert point_relation_rows_arg("point_relation", lines, pts, [0, 1, 2], False) is None  # the identity is no row map
    for a, b in ((PT, LS), (LS, PT), (MPT, MPG), (PG, MPT), (PT, PT)):
        for name, pred in POINT_RELATION_PREDICATES.items():
            assert point_relation_predicate_arg(name, a, b) == pred
    assert all(s._dev is None for s in (pts, two, lines, polys))


def test_table_joins_check_their_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    for opts in (SpatialJoinRelationArgs(join_type="outer"), SpatialJoinRelationArgs(predicate="contains_properly"), SpatialJoinRelationArgs(predicate="disjoint")):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            spatial_join_point_relation(t, t, opts)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    for kw in ({"join_type": "outer"}, {"predicate": "disjoint"}, {"predicate": "dwithin"}):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            sjoin(t, t, **kw)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_the_older_methods_still_refuse_a_point_column(no_device):
    pts, _, lines, polys = _series()
    for name in ("touches", "crosses", "covered_by", "covers", "disjoint"):
        for other in (polys, lines, pts):
            with pytest.raises(NotImplementedError, match="Point x"):
                getattr(pts, name)(other)
    for name in ("overlaps", "geom_equals", "contains_properly"):
        for other in (polys, pts):
            with pytest.raises(NotImplementedError, match="Point x"):
                getattr(pts, name)(other)
    for join in (relation_pairs, polygon_relation_pairs, line_relation_pairs):
        with pytest.raises(_abi.MismatchedGeometry):
            join(pts, polys, "touches")
