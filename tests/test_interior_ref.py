"""The exact reference of representative_point (tests/interior_ref.py) pinned on hand-computed cases, the fixture's reproducibility byte
for byte, and the fixture's promise: every non-degenerate polygonal row has its widest section at least 1e-6 of its diagonal wide and
the reference's midpoint strictly inside the polygon (tests/exact_predicates.py), at both placements."""
import os
from fractions import Fraction as F

import numpy as np
import pytest

from tests import exact_predicates as E
from tests import interior_ref as I
from tests.golden import make_interior_golden


@pytest.fixture(scope="module")
def golden():
    return np.load(I.GOLDEN)


def _sections(rings):
    return [(x0, x1) for x0, x1, _ in I.member_sections(rings)["sections"]]


def test_scan_line_by_hand():
    assert I.scan_y([I.L_SHAPE]) == 4.0  # ordinates 0, 2, 6: centre 3, lo 2, hi 6
    assert I.scan_y([I.TRI]) == 1.5  # 0, 3: lo stays miny, hi stays maxy
    assert I.scan_y([[(0, 0), (4, 2), (0, 4), (-4, 2), (0, 0)]]) == 3.0  # a vertex AT the centre is lo
    assert I.scan_y(I.RING_SHAPE) == 5.0  # the hole's ordinates 3 and 7 bracket the centre
    assert I.scan_y([[(0, 0), (5, 0), (2, 0), (0, 0)]]) == 0.0
    up = float(np.nextafter(1.0, 2.0))
    assert I.scan_y([[(0, 0), (6, 1), (3, 2), (-1, up), (0, 0)]]) in (1.0, up)  # adjacent doubles: the average is one of them


def test_sections_by_hand():
    assert _sections([I.L_SHAPE]) == [(0, 2)]
    assert _sections([I.U_SHAPE]) == [(0, 2), (4, 6)]
    assert _sections(I.RING_SHAPE) == [(0, 3), (7, 10)]
    assert _sections([I.TRI]) == [(0, 2)]  # at y = 1.5 the hypotenuse is at x = 2
    assert _sections(I.holed((2, 4), (15, 17))) == [(0, 2), (4, 15), (17, 20)]
    assert _sections([I.comb(3)]) == [(0, 1), (3, 4), (6, 7)]  # stored right to left, sorted by x
    assert len(I.member_sections([I.comb(17)])["crossings"]) == 34
    assert I.member_sections([[(0, 0), (2, 2), (4, 4), (0, 0)]])["sections"] == [(3, 3, 0)]


def test_upper_end_rule_by_hand():
    """scanY on a vertex: the edge that ends there from below is not counted, the one that leaves upwards is"""
    m = I.member_sections([[(0, 0), (6, 1), (3, 2), (-1, float(np.nextafter(1.0, 2.0))), (0, 0)]])
    assert m["scan"] == 1.0 and [e for _, e in m["crossings"]] == [3, 1] and m["crossings"][1][0] == 6


def test_choice_by_hand():
    r = I.polygon_row(I.PG, [I.U_SHAPE])
    assert r["choice"] == (0, 0) and r["max_width"] == 2  # the first of two equal sections
    sq = lambda x, w: [I.rect(x, 0, x + w, 4)]  # noqa: E731
    assert I.polygon_row(I.MPG, [sq(0, 5), [], sq(20, 5)])["choice"] == (0, 0)  # equal widths: the first member
    assert I.polygon_row(I.MPG, [sq(0, 2), [], sq(20, 8), sq(30, 5)])["choice"] == (1, 0)
    flat = I.polygon_row(I.PG, [[(0, 0), (2, 2), (4, 4), (0, 0)]])
    assert flat["choice"] is None and flat["first"] == (0.0, 0.0) and flat["max_width"] == 0
    assert I.polygon_row(I.MPG, [[], [[]]])["first"] is None


def test_vertex_rows_by_hand():
    r = I.vertex_row(I.LS, [(0, 0), (0, 2), (4, 2), (4, 0)])
    assert r["centroid"] == (2, F(3, 2)) and [(x, y) for x, y, _ in r["candidates"]] == [(0, 2), (4, 2)]
    assert r["candidates"][0][2] == r["candidates"][1][2] == F(17, 4)
    r = I.vertex_row(I.LS, [(0, 0), (4, 3)])  # no interior vertex: the end points
    assert [(x, y) for x, y, _ in r["candidates"]] == [(0, 0), (4, 3)] and r["centroid"] == (2, F(3, 2))
    r = I.vertex_row(I.MLS, [[(0, 0), (10, 0)], [], [(0, 5), (3, 5), (10, 5)]])
    assert [(x, y) for x, y, _ in r["candidates"]] == [(3, 5)] and r["centroid"] == (5, F(5, 2))
    r = I.vertex_row(I.MPT, [(0, 0), (4, 0), (4, 0), (10, 10)])
    assert r["centroid"] == (F(9, 2), F(5, 2)) and min(r["candidates"], key=lambda c: c[2])[:2] == (4, 0)
    assert I.vertex_row(I.MLS, [[], []]) is None and I.vertex_row(I.PT, None) is None


def test_fixture_is_reproducible_byte_for_byte(tmp_path):
    out = tmp_path / "interior_lattice.npz"
    make_interior_golden.main(str(out))
    assert out.read_bytes() == open(I.GOLDEN, "rb").read()
    assert os.path.getsize(I.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(I.GOLDEN), "overlay_lattice.npz"))


@pytest.mark.parametrize("fam", list(I.FAMILIES))
def test_recorded_verdicts_are_the_reference_s(golden, fam):
    """what the fixture records at the lattice placement is what the reference says about the fixture's columns today"""
    kind = I.FAMILIES[fam]
    rows = I.column_rows(I.fixture_column(golden, fam))
    if kind in (I.PG, I.MPG):
        refs = [I.polygon_row(kind, r) for r in rows]
        assert np.array_equal(golden[f"{fam}_scan"], [r["members"][0]["scan"] if r["members"] else np.nan for r in refs], equal_nan=True)
        assert np.array_equal(golden[f"{fam}_crossings"], [len(r["members"][0]["crossings"]) if r["members"] else -1 for r in refs])
        assert np.array_equal(golden[f"{fam}_width"], [float(r["max_width"]) for r in refs])
        w = dict(zip(golden[f"{fam}_names"], golden[f"{fam}_width"]))
        assert w["empty"] == 0 and (fam != "pg" or (w["u_shape"], w["ring_shape"], w["hole2_widest_middle"], w["flat_diagonal"]) == (2, 3, 11, 0))
    else:
        for r, want in zip(rows, golden[f"{fam}_nearest"]):
            ref = I.vertex_row(kind, r)
            if ref is None:
                assert np.isnan(want).all()
            else:
                d = min(c[2] for c in ref["candidates"])
                assert tuple(want) == next((c[0], c[1]) for c in ref["candidates"] if c[2] == d)


def test_degenerate_lines_take_geo_s_centroid():
    """no member of positive length: the members' starts, weighted by their segment counts; a zero-length member beside a real one is
    ignored"""
    r = I.vertex_row(I.MLS, [[(0, 0)] * 4, [], [(10, 0)] * 3, [(7, 7)]])
    assert r["centroid"] == (F(27, 6), F(7, 6)) and [c[:2] for c in r["candidates"]] == [(0, 0), (0, 0), (10, 0)]
    assert I.vertex_row(I.MLS, [[(100, 100)] * 3, [(0, 0), (2, 0), (4, 0)]])["centroid"] == (2, 0)
    assert I.vertex_row(I.LS, [(3, 1)] * 3)["centroid"] == (3, 1)


def test_fixture_holds_the_rows_the_kernel_paths_need(golden):
    names = set(golden["pg_names"])
    assert {f"comb_{k}" for k in (1, 2, 3, I.G_SMALL // 2, I.G_SMALL, I.G_LARGE // 2, I.G_LARGE, I.SLICE - 1, I.SLICE, I.SLICE + 1)} <= names
    col = I.fixture_column(golden, "pg")
    n = dict(zip(golden["pg_names"], np.diff(col.ring_offsets[col.geom_offsets])))
    assert n["triangle"] == 4 and n["comb_512"] == I.BLOCK_COORDS and n["comb_513"] == I.BLOCK_COORDS + 1 and n["comb_2048"] == 2048
    cr = dict(zip(golden["pg_names"], golden["pg_crossings"]))
    assert cr["comb_16"] == I.SLICE and cr["comb_17"] == I.SLICE + 2 and n["comb_17"] <= I.BLOCK_COORDS  # a queued row
    assert cr["comb_513"] == 200 and cr["comb_2048"] == 800  # the work-group path sorts hundreds of crossings
    assert cr["hole1_widest_first"] == 4 and cr["hole2_widest_middle"] == 6
    assert (n["u_shape_512"], n["u_shape_513"], cr["u_shape_512"], cr["u_shape_513"]) == (I.BLOCK_COORDS, I.BLOCK_COORDS + 1, 4, 4)  # few crossings, both kernels
    for fam in I.FAMILIES:
        assert not golden[f"{fam}_valid"][-1] and "empty" in set(golden[f"{fam}_names"]), fam


@pytest.mark.parametrize("placement", list(I.PLACEMENTS))
@pytest.mark.parametrize("fam", ["pg", "mpg"])
def test_reference_midpoint_is_strictly_inside(golden, fam, placement):
    """every non-degenerate row: widest section >= 1e-6 * diagonal (so the GPU test's interior guarantee excludes no row), and the
    midpoint of the reference's choice strictly inside the polygon"""
    kind = I.FAMILIES[fam]
    seen = 0
    for name, row, valid in zip(golden[f"{fam}_names"], I.column_rows(I.fixture_column(golden, fam, I.PLACEMENTS[placement])), golden[f"{fam}_valid"]):
        ref = I.polygon_row(kind, row)
        if not valid or ref["choice"] is None:
            continue
        assert ref["max_width"] >= F(I.MIN_REL_WIDTH * I.diagonal(kind, row)), name
        m, k = ref["choice"]
        x0, x1, _ = ref["members"][m]["sections"][k]
        p = np.array([float((x0 + x1) / 2), ref["members"][m]["scan"]])  # (rounded where the midpoint is no double)
        assert E.point_predicate(p, I.live_members(kind, row), "contains"), name
        seen += 1
    assert seen >= 10


def test_adjacent_ordinates_survive_the_georeferenced_placement(golden):
    col = I.fixture_column(golden, "pg", I.OFFSET)
    row = I.column_rows(col)[list(golden["pg_names"]).index("adjacent_georeferenced")]
    ys = sorted({p[1] for p in row[0]})
    assert ys[2] == np.nextafter(ys[1], np.inf) and I.scan_y(row) in (ys[1], ys[2])
