"""GPU: every exact family on rows where the stage-A orientation filter gives up although the exact sign is NOT zero.

The fixtures are those of tests/hard_orient.py (what they promise is checked without a GPU in tests/test_hard_orient.py): of every 8
rows 4 carry a triple (a, b, c) on which the sign of the double determinant is wrong under all six argument orders, 2 one on which the
filter is uncertain but the double sign right, 1 is exactly collinear at wide mantissas, 1 is easy.  Far points make the planted sign
the one thing that decides a row's answer, so a kernel whose exact arm is wrong, is missing, or is by-passed by a floating short cut
gives other masks, pairs, codes or triangles than the exact references.  Everything is compared exactly.

Each test asserts the lane-group size or the kernel path it claims to select."""
import ctypes as C
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialIndex,
    join_pairs,
    line_relation_pairs,
    point_relation_pairs,
    polygon_relation_pairs,
    relation_pairs,
)
from tests import exact_predicates as E
from tests import exact_ref as X
from tests import hard_orient as H
from tests import linerel_ref as L
from tests import pointrel_ref as P
from tests import polyrel_ref as Y
from tests import relation_ref as R
from tests import triangulate_ref as T
from tests import validity_ref as V

pytestmark = pytest.mark.gpu

PT, MPT, LS, MLS, PG, MPG = P.PT, P.MPT, P.LS, P.MLS, P.PG, P.MPG
GENS = sorted(H.GENERATORS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LONG = 64  # rows of the columns built from 48-coordinate rings (the larger lane group): the first 8 blocks of the composition


def series(kind, rows):
    return GeoSeries(X.column(kind, rows))


def mean_coords(s: GeoSeries) -> float:
    return s.array.n_coords / max(s.array.n_geoms, 1)


def assert_equal(got, want, rows, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    assert len(bad) == 0, (what, [(int(i), rows[i].kind, int(got[i]), int(want[i])) for i in bad[:8]], len(bad))


def planted(rows, by_sign):
    """the answers the construction promises, from the exact sign of the planted triple: {+1: .., 0: .., -1: ..}"""
    return np.array([by_sign[t.sign] for t in rows])


# ---- point in polygon, row-wise: dev::ring_edge -> dev::orient2d -> orient2d_exact --------------------------------------------------------


def ballast_ring(n_coords: int):
    """a valid ring of n_coords coordinates far from every fixture (all of them lie within 2^36 of the origin)"""
    b, s = 2.0**40, 2.0**10
    k = n_coords - 3
    return [(b + i * s, b) for i in range(k)] + [(b + (k - 1) * s, b + s), (b, b + s), (b, b)]


def pip_expected(polys, pts):
    w = np.array([E.point_predicate(np.array(p), [g], "within") for g, p in zip(polys, pts)])
    i = np.array([E.point_predicate(np.array(p), [g], "intersects") for g, p in zip(polys, pts)])
    return w, i


@pytest.mark.parametrize("gen", GENS)
def test_rowwise_point_in_polygon(gpk, gen):
    """contains / within / intersects at G = 1, 2 and 16 of point_poly_predicate_kernel (ballast rows that no pair names lift the
    column's mean), on rings of 48 coordinates with the planted edge in the middle (G = 4: the lanes stride over the edges), with the
    ring started elsewhere, and under the exact symmetries"""
    rows = H.triples(gen)
    polys, pts = [H.polygon_row(t) for t in rows], [t.c for t in rows]
    within, inter = pip_expected(polys, pts)
    assert np.array_equal(within, planted(rows, {1: True, 0: False, -1: False})) and np.array_equal(inter, planted(rows, {1: True, 0: True, -1: False}))
    n = len(rows)
    sq = series(PT, pts)
    seen = set()
    for G, k, coords in ((1, 0, 0), (2, 8, 513), (16, 8, 4097)):
        sp = series(PG, polys + [[ballast_ring(coords)]] * k)
        assert E.pick_group_rows(sp.array.n_coords, sp.array.n_geoms) == G
        seen.add(G)
        idx = np.arange(n, dtype=np.uint32)
        assert_equal(sq.within(sp, other_rows=idx), within, rows, ("within", G))
        assert_equal(sq.intersects(sp, other_rows=idx), inter, rows, ("intersects", G))
        back = np.concatenate([idx, np.zeros(k, dtype=np.uint32)])  # (a ballast polygon against point 0: far away)
        assert_equal(sp.contains(sq, other_rows=back)[:n], within, rows, ("contains", G))
        assert not sp.contains(sq, other_rows=back)[n:].any()
    for shift in (0, 1, 24):  # the planted edge first, last (it closes the ring) and in the middle of the ring
        long_polys = [[H.rotated(H.polygon_row(t, long=True)[0], shift)] for t in rows]
        sp = series(PG, long_polys)
        assert E.pick_group_rows(sp.array.n_coords, sp.array.n_geoms) == 4
        seen.add(4)
        assert_equal(sq.within(sp), within, rows, ("within, long rings", shift))
        assert_equal(sp.contains(sq), within, rows, ("contains, long rings", shift))
        assert_equal(sq.intersects(sp), inter, rows, ("intersects, long rings", shift))
    assert seen == {1, 2, 4, 16}
    for name, f in H.SYMMETRIES.items():
        moved = [f(t) for t in rows]
        mp, mq = [H.polygon_row(t) for t in moved], [t.c for t in moved]
        w, i = pip_expected(mp, mq)
        assert (w != within).any() or name.startswith("scale")  # (a mirror turns inside into outside)
        assert_equal(series(PT, mq).within(series(PG, mp)), w, moved, ("within", name))
        assert_equal(series(PG, mp).intersects(series(PT, mq)), i, moved, ("intersects", name))


# ---- the point join: ring_edge_flat (one launch), ring_edge_filtered (chain kernel), and the exact walk both hand over to ---------------------


@lru_cache(maxsize=None)
def fan_expected():
    """(pairs sorted by (point, polygon), counts): a point joins the polygons it lies strictly inside (gpk_spatial_join evaluates
    poly.contains(point)), by exact_predicates.point_predicate"""
    polys, pts = H.fan_polygons(), H.fan_points()
    P_ = np.array(pts)
    hit = np.zeros((len(pts), len(polys)), dtype=bool)
    for j, g in enumerate(polys):  # (a point outside a polygon's box is outside the polygon: an exact statement)
        ring = np.array(g[0])
        near = np.nonzero((P_ >= ring.min(axis=0)).all(axis=1) & (P_ <= ring.max(axis=0)).all(axis=1))[0]
        hit[near, j] = [E.point_predicate(P_[i], [g], "contains") for i in near]
    ll, rr = np.nonzero(hit)
    return np.stack([ll, rr], axis=1).astype(np.uint32), hit.sum(axis=1).astype(np.uint32)


def join_stats(fn):
    """fn() with the join statistics on: (result, rows listed for the exact step, chain edges evaluated there, rows handed to the walk)"""
    lib = _abi.lib()
    st = (C.c_int64 * 4)()
    lib.gpk_join_stats_enable(1)
    lib.gpk_join_stats(st, 1)
    try:
        out = fn()
        lib.gpk_join_stats(st, 1)
    finally:
        lib.gpk_join_stats_enable(0)
    return out, int(st[0]), int(st[1]), int(st[2])


def fan_join_check():
    """the join of the fan's points and polygons in this process (whatever tile kernel its environment selects) against the exact
    pairs; returns the index's description and the statistics of the planted run and of its easy twin"""
    polys, pts = H.fan_polygons(), H.fan_points()
    want_pairs, want_counts = fan_expected()
    kinds = [t.kind for t, _ in H.fan()]
    uncertain = [i for i, k in enumerate(kinds) if k != H.EASY]
    # (the construction: a planted point is inside its own polygon exactly when it is left of a -> b, and inside no other)
    own = {int(l) for l, r in want_pairs if l == r and l < H.FAN_N}
    assert own == {i for i, (t, _) in enumerate(H.fan()) if t.sign > 0}
    right = series(PG, polys)
    index = SpatialIndex(right)
    d = index.describe()
    (pairs, counts), listed, edges, walked = join_stats(lambda: join_pairs(series(PT, pts), right, "intersects", r_index=index))
    assert np.array_equal(counts, want_counts), [(int(i), kinds[i] if i < H.FAN_N else "-", int(counts[i]), int(want_counts[i])) for i in np.nonzero(counts != want_counts)[0][:8]]
    assert np.array_equal(pairs, want_pairs)
    # the twin: every planted point 1 / 2000 of the edge's length off it (certain; some 0.02 away), everything else the same
    twin = list(pts)
    for i in uncertain:
        t = H.fan()[i][0]
        twin[i] = H.at(t, H.along(t), 0.0005 if t.sign >= 0 else -0.0005)
        assert H.kind_of(t.a, t.b, twin[i]) == H.EASY
    (_, tcounts), tlisted, tedges, twalked = join_stats(lambda: join_pairs(series(PT, twin), right, "intersects", r_index=index))
    assert np.array_equal(tcounts[H.FAN_N :], want_counts[H.FAN_N :])
    return d, (listed, edges, walked), (tlisted, tedges, twalked), len(uncertain)


def fan_path_assertions(d, stats, twin_stats, n_uncertain):
    """the index is lean with chains and a routing image (so the process's tile kernel — the one-launch join, or the chain kernel under
    GPK_TILE_KERNEL=chain — served the join), the planted points were test points of half cells with a chain, and the filter sent them
    to the exact walk: the twin column, equal but for its certain points, hands over fewer rows by most of the uncertain ones (a planted
    point in a list cell near the fan's centre, or in a half cell without a chain, is walked in both runs)"""
    assert d["lean"] and d["chains"] and d["route"], d
    listed, edges, walked = stats
    _, tedges, twalked = twin_stats
    assert listed >= H.FAN_N // 2 and edges > 0 and tedges > 0, (stats, twin_stats)
    assert walked - twalked >= n_uncertain // 2, (stats, twin_stats, n_uncertain)


def test_point_join_one_launch(gpk, oracle):
    """ring_edge_flat and the walk of the one-launch join (gpk_pipflow.hip): hard points in boundary cells; the first polygon of every
    quadrant is 16 degrees wide and has interior cells, its planted point lies at its edge all the same"""
    assert os.environ.get("GPK_TILE_KERNEL") != "chain"
    d, stats, twin_stats, n_uncertain = fan_join_check()
    print("one-launch join:", d, stats, twin_stats, n_uncertain)
    fan_path_assertions(d, stats, twin_stats, n_uncertain)
    polys, pts = X.column(PG, H.fan_polygons()), X.column(PT, H.fan_points())
    exp_pairs, exp_counts, _ = oracle.spatial_join(pts, polys, "intersects", mode=0)  # (the CPU oracle agrees with the exact pairs)
    assert np.array_equal(exp_pairs, fan_expected()[0]) and np.array_equal(exp_counts, fan_expected()[1])
    # interior cells exist: a centroid of a wide polygon is settled without the exact step in a run of the centroids alone
    wide = [H.FAN_N + i for i in range(0, H.FAN_N, H.FAN_N // 4)]
    right = series(PG, H.fan_polygons())
    (_, counts), listed, _, walked = join_stats(lambda: join_pairs(series(PT, [H.fan_points()[i] for i in wide]), right, "intersects"))
    assert counts.tolist() == [1, 1, 1, 1] and listed == 0 and walked == 0, (counts, listed, walked)


def test_point_join_chain_kernel(gpk):
    """ring_edge_filtered and the exact pass of pip_tile_chain_kernel (gpk_join.hip): GPK_TILE_KERNEL is read once per process, so the
    same check runs in its own interpreter"""
    prog = (
        "import os, sys\nsys.path.insert(0, os.getcwd())\n"
        "from tests.test_gpu_hard_orient import fan_join_check, fan_path_assertions\n"
        "out = fan_join_check()\nprint('chain kernel:', out)\nfan_path_assertions(*out)\nprint('CHAIN_OK')\n"
    )
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, GPK_TILE_KERNEL="chain"))
    assert r.returncode == 0 and "CHAIN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout[-600:])


# ---- the four relation-mask families ------------------------------------------------------------------------------------------------------------


def grid_masks(fn, ka, rows_a, kb, rows_b):
    """row-wise masks of a reference that works on integers (relation_ref, polyrel_ref): each pair on its own exact integer grid"""
    out = np.zeros(len(rows_a), dtype=np.uint8)
    for i, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        a, b = H.on_integer_grid(ra, rb)
        out[i] = fn(ka, a, kb, b)
    return out


def box_of(row):
    flat = []

    def walk(r):
        if isinstance(r, tuple) and not isinstance(r[0], (tuple, list)):
            flat.append(r)
        else:
            for q in r:
                walk(q)

    walk(row)
    a = np.array(flat)
    return a.min(axis=0), a.max(axis=0)


def mask_table(fn, ka, rows_a, kb, rows_b, apart: int):
    """the exact masks of every row of A against every row of B: `apart` where the boxes are apart, fn on an integer grid elsewhere"""
    ba, bb = [box_of(r) for r in rows_a], [box_of(r) for r in rows_b]
    table = np.full((len(rows_a), len(rows_b)), apart, dtype=np.uint8)
    n = 0
    for i, (alo, ahi) in enumerate(ba):
        for j, (blo, bhi) in enumerate(bb):
            if (alo <= bhi).all() and (blo <= ahi).all():
                a, b = H.on_integer_grid(rows_a[i], rows_b[j])
                table[i, j] = fn(ka, a, kb, b)
                n += 1
    assert len(rows_a) <= n <= len(rows_a) * H.PER_CLASS  # every block of PER_CLASS rows at its own scale: only its own rows can be candidates
    return table


def join_checks(abi_name, pairs_fn, sa, sb, expected, pred_ids, what):
    """the join's refine with pairs and masks, and count-only (its early-exit form), for every predicate"""
    for pred, pid in pred_ids.items():
        p0, c0, m0 = expected(pred)
        pairs, counts, masks = pairs_fn(sa, sb, pred)
        assert np.array_equal(pairs, p0) and np.array_equal(counts, c0) and np.array_equal(masks, m0), (what, pred, len(pairs), len(p0))
        n = C.c_int64(-1)
        only = np.zeros(len(sa), dtype=np.uint32)
        rc = getattr(_abi.lib(), abi_name)(sa.device().handle, sb.device().handle, None, pid, 0, only.ctypes.data, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
        assert rc == _abi.GPK_OK and n.value == len(p0) and np.array_equal(only, c0), (what, pred, n.value, len(p0))
    assert any(len(expected(p)[0]) >= len(sa) // 8 for p in pred_ids), what  # (a point is on a line only in the collinear rows: one in eight)


def lanes(group_fn, *cols, long):
    assert group_fn(*cols) == (16 if long else 4), [mean_coords(c) for c in cols]


@pytest.mark.parametrize("long", [False, True], ids=["G4", "G16"])
@pytest.mark.parametrize("gen", GENS)
def test_point_relation(gpk, gen, long):
    """gpk_point_relation: c against the line [a, b] and against the polygon (a, b, r), as a POINT and in a MULTIPOINT with a far point"""
    from tests.test_gpu_pointrel import lanes_of

    rows = H.triples(gen)[: N_LONG if long else H.N_ROWS]
    jrows = H.placed_triples(gen)
    for ka, kb in ((PT, LS), (PT, PG), (MPT, LS), (MPT, PG)):
        A = lambda ts: [t.c if ka == PT else H.probe_points(t) for t in ts]  # noqa: E731
        B = lambda ts: [H.line_row(t, long) if kb == LS else H.polygon_row(t, long) for t in ts]  # noqa: E731
        sa, sb = series(ka, A(rows)), series(kb, B(rows))
        lanes(lanes_of, sa, sb, long=long)
        want = P.masks(ka, A(rows), kb, B(rows))
        far = 0 if ka == PT else 4  # (the far point of the MULTIPOINT is outside B)
        by = {(LS, 1): 12, (LS, 0): 9, (LS, -1): 12, (PG, 1): 9, (PG, 0): 10, (PG, -1): 12}
        assert np.array_equal(want, planted(rows, {s: by[kb, s] | far for s in (1, 0, -1)}))
        assert_equal(sa.point_relation(sb), want, rows, (ka, kb))
        assert_equal(sb.point_relation(sa), want, rows, (ka, kb, "swapped"))  # (the punctual side stays A)
        ja, jb = A(jrows), B(jrows)
        ones = np.ones(len(jrows), dtype=bool)
        table = P.mask_table(ka, ja, ones, kb, jb, ones)
        sja, sjb = series(ka, ja), series(kb, jb)
        lanes(lanes_of, sja, sjb, long=long)
        join_checks("gpk_point_relation_join", point_relation_pairs, sja, sjb, lambda pred: P.expected_pairs(table, pred, P.DIM[kb]), P.PRED_IDS, (ka, kb))


@pytest.mark.parametrize("long", [False, True], ids=["G4", "G16"])
@pytest.mark.parametrize("gen", GENS)
def test_line_relation(gpk, gen, long):
    """gpk_line_relation: [a, b] against [c, q] — a proper crossing, an end inside the other line, or nothing shared"""
    from tests.test_gpu_linerel import lanes_of

    rows = H.triples(gen)[: N_LONG if long else H.N_ROWS]
    A, B = [H.line_row(t, long) for t in rows], [H.probe_line(t) for t in rows]
    sa, sb = series(LS, A), series(LS, B)
    lanes(lanes_of, sa, sb, long=long)
    want = L.masks(LS, A, LS, B)
    assert len(set(want.tolist())) == 3 and np.array_equal(want, planted(rows, {s: int(want[[t.sign for t in rows].index(s)]) for s in (1, 0, -1)}))
    assert_equal(sa.line_relation(sb), want, rows, "a x b")
    assert_equal(sb.line_relation(sa), L.swapped(want), rows, "b x a")
    jrows = H.placed_triples(gen)
    ja, jb = [H.line_row(t, long) for t in jrows], [H.probe_line(t) for t in jrows]
    ones = np.ones(len(jrows), dtype=bool)
    table = L.mask_table(LS, ja, ones, LS, jb, ones)
    sja, sjb = series(LS, ja), series(LS, jb)
    lanes(lanes_of, sja, sjb, long=long)
    join_checks("gpk_line_relation_join", line_relation_pairs, sja, sjb, lambda pred: L.expected_pairs(table, pred), L.PRED_IDS, "line x line")


@pytest.mark.parametrize("long", [False, True], ids=["G4", "G16"])
@pytest.mark.parametrize("gen", GENS)
def test_line_polygon_relation(gpk, gen, long):
    """gpk_line_polygon_relation (gpk_linearea.hip): [c, q] against (a, b, r) — crosses, touches, disjoint"""
    from tests.test_gpu_relation import lanes_of

    rows = H.triples(gen)[: N_LONG if long else H.N_ROWS]
    A, B = [H.probe_line(t) for t in rows], [H.polygon_row(t, long) for t in rows]
    sa, sb = series(LS, A), series(PG, B)
    lanes(lanes_of, sb, long=long)
    want = grid_masks(R.mask, LS, A, PG, B)
    assert np.array_equal(want, planted(rows, {1: 7, 0: 6, -1: 4}))
    assert_equal(sa.line_polygon_relation(sb), want, rows, "line x polygon")
    assert_equal(sb.line_polygon_relation(sa), want, rows, "polygon x line")  # (either order of the two families: the same mask)
    jrows = H.placed_triples(gen)
    ja, jb = [H.probe_line(t) for t in jrows], [H.polygon_row(t, long) for t in jrows]
    table = mask_table(R.mask, LS, ja, PG, jb, apart=R.EXTERIOR)
    sja, sjb = series(LS, ja), series(PG, jb)
    lanes(lanes_of, sjb, long=long)
    join_checks("gpk_line_polygon_join", relation_pairs, sja, sjb, lambda pred: R.expected_pairs(table, pred), R.PRED_IDS, "line x polygon")


@pytest.mark.parametrize("long", [False, True], ids=["G4", "G16"])
@pytest.mark.parametrize("gen", GENS)
def test_polygon_relation(gpk, gen, long):
    """gpk_polygon_relation: the triangle (c, q2, q1) against (a, b, r) on the other side of a -> b — overlaps, touches, disjoint"""
    from tests.test_gpu_polyrel import lanes_of

    rows = H.triples(gen)[: N_LONG if long else H.N_ROWS]
    A, B = [H.probe_triangle(t) for t in rows], [H.polygon_row(t, long) for t in rows]
    sa, sb = series(PG, A), series(PG, B)
    lanes(lanes_of, sa, sb, long=long)
    want = grid_masks(Y.mask, PG, A, PG, B)
    assert np.array_equal(want, planted(rows, {1: 15, 0: 14, -1: 12}))
    assert_equal(sa.polygon_relation(sb), want, rows, "a x b")
    assert_equal(sb.polygon_relation(sa), Y.swapped(want), rows, "b x a")
    jrows = H.placed_triples(gen)
    ja, jb = [H.probe_triangle(t) for t in jrows], [H.polygon_row(t, long) for t in jrows]
    table = mask_table(Y.mask, PG, ja, PG, jb, apart=Y.A_OUTSIDE | Y.B_OUTSIDE)
    sja, sjb = series(PG, ja), series(PG, jb)
    lanes(lanes_of, sja, sjb, long=long)
    join_checks("gpk_polygon_relation_join", polygon_relation_pairs, sja, sjb, lambda pred: Y.expected_pairs(table, pred), Y.PRED_IDS, "polygon x polygon")


# ---- validity and simplicity ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("long", [False, True], ids=["G4", "G16"])
@pytest.mark.parametrize("gen", GENS)
def test_validity_and_simplicity(gpk, gen, long):
    """the shell carries a -> b and a hole, or a second member, has a vertex at c; a line's vertex c sits beside another of its segments
    or beside a segment of another member"""
    rows = H.triples(gen)[: N_LONG if long else H.N_ROWS]
    for kind, build in ((PG, H.hole_row), (MPG, H.members_row)):
        col = [build(t, long) for t in rows]
        codes, where = V.validity_column(kind, col)
        assert V.lanes_of(sum(V.n_coords(kind, r) for r in col), len(col)) == (V.VAL_G_LARGE if long else V.VAL_G_SMALL)
        assert {V.VALID, V.RINGS_CROSS} <= set(codes.tolist())
        for t, c in zip(rows, codes):  # the planted sign decides (an easy row, a tenth of the edge off it, may have its hole outside)
            if t.kind != H.EASY and kind == MPG:
                assert c == (V.RINGS_CROSS if t.sign > 0 else V.VALID)
        got_c, got_w = series(kind, col).is_valid_reason(return_where=True)
        assert_equal(got_c, codes, rows, ("codes", kind))
        assert_equal(got_w, where, rows, ("where", kind))
    for kind, build in ((LS, H.self_line_row), (MLS, H.two_lines_row)):
        col = [build(t, long) for t in rows]
        want = V.is_simple_column(kind, col)
        assert V.lanes_of(sum(V.n_coords(kind, r) for r in col), len(col)) == (V.VAL_G_LARGE if long else V.VAL_G_SMALL)
        assert np.array_equal(want, planted(rows, {1: True, 0: False, -1: False}))
        assert_equal(series(kind, col).is_simple(), want, rows, ("is_simple", kind))


# ---- triangulation: tri::orient -> tri::orient_exact, on the device and on the host -------------------------------------------------------------


@pytest.fixture(scope="module")
def host_answers(tmp_path_factory):
    """tests/triangulate_host_driver.cpp built with the host compiler, as tests/test_triangulate_host.py builds it: a function
    (kind, rows) -> [(status, row-local triangles)]"""
    from tests.host_build import compilers
    from tests.test_triangulate_host import run

    out = tmp_path_factory.mktemp("hard_orient_driver")
    exe = str(out / "triangulate_driver")
    log = []
    for cxx in compilers():
        r = subprocess.run([cxx, "-std=c++17", "-ffp-contract=off", "-O2", f"-I{os.path.join(ROOT, 'geopolars_amd', 'csrc')}",
                            os.path.join(ROOT, "tests", "triangulate_host_driver.cpp"), "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return lambda kind, rows: run(exe, out, kind, rows)
        log.append(f"{cxx}: {r.stderr[-400:]}")
    raise AssertionError("no host compiler built the driver:\n" + "\n".join(log))


def triangulation_rows(gen, long):
    """(rows, the triples they come from): c as a vertex between a and b (reflex, convex or collinear by the planted sign), c beside the
    diagonal a - b of an ear, and c as the hole vertex the bridge starts from, a hard margin inside the cone at a; long: the shells of
    the hole rows have 48 coordinates (the larger lane group)"""
    ts = H.triples(gen)[: N_LONG if long else H.N_ROWS]
    if long:
        return [H.hole_row(t, True) for t in ts], list(ts)
    return [f(t) for t in ts for f in (H.chain_row, H.notch_row, H.hole_row)], [t for t in ts for _ in range(3)]


@pytest.mark.parametrize("long", [False, True], ids=["G4", "G16"])
@pytest.mark.parametrize("gen", GENS)
def test_triangulation(gpk, host_answers, gen, long):
    from tests.test_gpu_triangulate import answers, bases, check_column, group_of

    rows, ts = triangulation_rows(gen, long)
    assert group_of(PG, rows) == (T.TRI_G_LARGE if long else T.TRI_G_SMALL)
    codes = V.validity_column(PG, rows)[0]
    # every chain and notch row is valid whatever the sign; a hole row is valid unless c lies an ulp (or a tenth) beyond the edge
    n_valid = int((codes == V.VALID).sum())
    assert n_valid >= (len(rows) // 4 if long else len(rows) * 3 // 4) and (codes != V.VALID).sum() >= len(rows) // 16
    got = answers(PG, rows)
    assert check_column(PG, rows, None, codes, got) == n_valid
    off, idx, st = got
    base = bases(PG, rows)
    host = host_answers(PG, rows)
    for i, (hs, htris) in enumerate(host):  # host and device: one rule, identical indices
        assert hs == st[i] and np.array_equal(idx[off[i] : off[i + 1]].astype(np.int64) - base[i], htris), (i, ts[i].kind, hs, int(st[i]))


# ---- convex hull ----------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("gen", GENS)
def test_convex_hull(gpk, oracle, gen):
    """{a, b, c, far}: c is a hull vertex only when it is right of a -> b; sets of 8 and of all 192 triples with their far points (the
    hard triples then lie inside the hull, but the sort and both chains still pass them); and the points of 192 rows as one LINESTRING"""
    rows = H.triples(gen)
    sets = [H.hull_row(t) for t in rows]
    sets += [[p for t in rows[i : i + 8] for p in H.hull_row(t)] for i in range(0, len(rows), 8)]
    sets += [[p for t in rows[i : i + 24] for p in H.hull_row(t)] for i in range(0, len(rows), 24)]
    sets += [[p for t in rows for p in H.hull_row(t)], [p for t in rows[::-1] for p in (t.c, t.b, t.a)]]
    # gpk_hull.hip: up to 64 points a row (hull_small_kernel), 65 .. HULL_CAP = 128 (the listed form), beyond (the work-group sort and
    # the one-lane chain)
    assert sorted({len(s) for s in sets}) == [4, 32, 96, 576, 768]
    col = X.column(MPT, sets)
    hx, ho = oracle.convex_hull(col)
    h = GeoSeries(col).convex_hull().array
    assert np.array_equal(h.ring_offsets, ho)
    sizes = set()
    for i, s in enumerate(sets):
        want = X.exact_hull(s)
        assert np.array_equal(X.canon(hx[ho[i] : ho[i + 1]]), X.canon(want)), i  # (the oracle is exact here too)
        got = h.xy[h.ring_offsets[i] : h.ring_offsets[i + 1]]
        assert np.array_equal(X.canon(got), X.canon(want)), (i, rows[i].kind if i < len(rows) else "-", len(got), len(want))
        if i < len(rows):
            assert len(want) - 1 == (4 if rows[i].sign < 0 else 3)
            sizes.add(len(want) - 1)
    assert sizes == {3, 4}


# ---- distance and dwithin at 0: held to what include/geopolars_hip.h states ----------------------------------------------------------------------------


def pair_group(a: GeoSeries, b: GeoSeries) -> int:
    """gpk_pairdist.h pairdist_group_size, restated: 32 lanes a row from a mean of 128 coordinates a row on the longer side, else 8"""
    return 32 if max(mean_coords(a), mean_coords(b)) >= 128.0 else 8


@pytest.mark.parametrize("mode", ["short", "long", "ballast"])
@pytest.mark.parametrize("gen", GENS)
def test_distance_zero_iff_the_sets_meet(gpk, gen, mode):
    """pairs of non-point columns (gpk_pairdist.hip): "0.0 exactly when A and B intersect as closed point sets, decided with exact
    orientations ... a disjoint pair is never 0: a vertex one ulp off a segment gives a tiny positive distance".  [a, b] against [c, q]
    crosses, touches or misses by a hard margin; the MULTIPOINT {c} is on [a, b] only in the collinear rows; {c} against the polygon
    (a, b, r) is 0 from the edge inwards.  dwithin(., 0) says the same.  short and long rows: 8 lanes a row, both argument orders;
    ballast: rows of 4097 coordinates that no pair names in the second column, 32 lanes a row."""
    long = mode == "long"
    rows = H.triples(gen)[: N_LONG if long else H.N_ROWS]
    k = 8 if mode == "ballast" else 0
    heavy = ballast_ring(4097)
    lines = series(LS, [H.line_row(t, long) for t in rows] + [heavy] * k)
    polys = series(PG, [H.polygon_row(t, long) for t in rows] + [[heavy]] * k)
    probes = series(LS, [H.probe_line(t) for t in rows])
    probes_b = series(LS, [H.probe_line(t) for t in rows] + [heavy] * k)
    single = series(MPT, [[t.c] for t in rows])
    first = series(LS, [H.line_row(t, long) for t in rows])
    sign = np.array([t.sign for t in rows])
    idx = np.arange(len(rows), dtype=np.uint32) if k else None
    for a, b, meets, what in ((first, probes_b, sign >= 0, "line x line"), (single, lines, sign == 0, "multipoint x line"), (single, polys, sign >= 0, "multipoint x polygon"),
                              (probes, polys, sign >= 0, "line x polygon")):
        assert pair_group(a, b) == (32 if k else 8), (what, mean_coords(a), mean_coords(b))
        for x, y in ((a, b),) if k else ((a, b), (b, a)):
            d = x.distance(y, other_rows=idx)
            assert not np.isnan(d).any() and (d >= 0).all()
            assert_equal(d == 0.0, meets, rows, (what, "distance == 0"))
            assert_equal(x.dwithin(y, 0.0, other_rows=idx), meets, rows, (what, "dwithin 0"))


@pytest.mark.parametrize("gen", GENS)
def test_point_distance_near_an_edge_is_counted(gpk, gen):
    """the POINT kernels (geo's EuclideanDistance per family) round their differences, and the header promises no exact zero for
    them: only the collinear rows are asserted (a point ON the line is at 0.0); of the others, how many come out as 0.0 is printed.
    Measured on MI355X: 144 of the 168 points off the line, in each of the three columns — all 96 hard and all 48 unsure rows: these
    kernels give 0.0 within a few ulps of a segment (geo's rule, as the CPU oracle applies it)."""
    rows = H.triples(gen)
    pts, lines = series(PT, [t.c for t in rows]), series(LS, [H.line_row(t) for t in rows])
    d = pts.distance(lines)
    sign = np.array([t.sign for t in rows])
    assert (d[sign == 0] == 0.0).all() and not np.isnan(d).any() and (d >= 0).all()
    off = sign != 0
    print(f"point x line, {gen}: {int((d[off] == 0.0).sum())} of {int(off.sum())} points off the line are at distance 0.0 (largest {d[off].max():.3g})")
