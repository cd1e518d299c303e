"""No GPU: what tests/hard_orient.py promises, checked on the references alone.

  1. the replica's constant and FILTER_SITES match geopolars_amd/csrc, and every named test exists;
  2. every column a GPU test uses has exactly the stated composition, survives the exact symmetries, and its far points are certain;
  3. the planted sign alone decides every family's answer, and each exact reference run with `sign(double determinant)` in place of
     its orientation gives another answer on at least half of the hard rows;
  4. a census of the inexact fixtures the suite had before (printed, not asserted);
  5. the figures for the constructive kernels (tests/hard_clip.py): composition, certainty of everything but the planted triple, the
     transition gap by the headers' definition, one shape per exact sign, and different shapes for + and -."""
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import exact_predicates as E
from tests import exact_ref as X
from tests import hard_clip as K
from tests import hard_orient as H
from tests import lineclip_ref as LC
from tests import linerel_ref as L
from tests import pointrel_ref as P
from tests import polyclip_ref as C
from tests import polyrel_ref as Y
from tests import polyunion_ref as U
from tests import relation_ref as R
from tests import triangulate_ref as T
from tests import validity_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENS = sorted(H.GENERATORS)


# ---- 1. the sources ----------------------------------------------------------------------------------------------------------------------


def test_constant_and_filter_sites_match_the_sources():
    """a sixth stage-A filter in csrc fails here until it is entered in hard_orient.FILTER_SITES with the test that reaches it"""
    counted, constants = H.counted_filter_sites()
    assert constants == {repr(H.STAGE_A)} and float(next(iter(constants))) == H.STAGE_A
    assert counted == H.inventory_filter_sites() and sum(counted.values()) == len(H.FILTER_SITES) == 5
    for s in H.FILTER_SITES:
        with open(os.path.join(H.CSRC, s.file)) as f:
            assert re.search(rf"\b{re.escape(s.function.split('::')[-1])}\(", f.read()), s


def test_filter_sites_name_tests_that_exist():
    for s in H.FILTER_SITES:
        if s.test is None:
            assert s.exempt and s.note, s
            continue
        assert not s.exempt, s
        path, name = s.test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(rf"^def {re.escape(name)}\(", f.read(), re.M), s.test


def test_the_dead_site_is_dead():
    """ring_edge_inline is exempt because nothing instantiates its only caller with INLINE_EXACT = true: if that changes, it needs a test"""
    text = ""
    for fn in sorted(os.listdir(H.CSRC)):
        if fn.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(H.CSRC, fn)) as f:
                text += f.read()
    assert len(re.findall(r"\bring_edge_inline\(", text)) == 2  # its definition and the INLINE_EXACT arm of chain_generic_row
    assert re.findall(r"chain_generic_row<(\w+)>", text) and set(re.findall(r"chain_generic_row<(\w+)>", text)) == {"false"}


def test_replica_against_the_rational_sign():
    """stage A never certifies a wrong sign, and kind_of's one-evaluation short cut agrees with the six classes"""
    rng = np.random.default_rng(3)
    seen = set()
    for gen in GENS:
        for kind in H.KINDS:
            for _ in range(60):
                a, b, c = H.GENERATORS[gen](kind, rng)
                cl = H.classes(a, b, c)  # (classify asserts the filter's promise for every certain evaluation)
                k = H.kind_of(a, b, c)
                seen.add(k)
                if k in H.HARD:
                    assert cl == "WWWWWW" and H.exact(a, b, c) == (1 if k == H.HARD_LEFT else -1)
                elif k == H.UNSURE:
                    assert cl == "UUUUUU"
                elif k == H.COLLINEAR:
                    assert cl == "ZZZZZZ" and H.uncertain_everywhere(a, b, c)
                elif k == H.EASY:
                    assert cl == "FFFFFF"
                else:
                    assert len(set(cl)) > 1 or cl == "ZZZZZZ"
    assert seen >= set(H.KINDS)


# ---- 2. the columns -------------------------------------------------------------------------------------------------------------------------


def columns():
    for gen in GENS:
        yield f"triples({gen})", H.triples(gen)
        yield f"placed_triples({gen})", H.placed_triples(gen)
    yield "fan", tuple(t for t, _ in H.fan())


@pytest.mark.parametrize("gen", GENS)
def test_compositions_are_exact(gen):
    """the condition that keeps a GPU test from being vacuous: classified anew, not by the rows' labels"""
    for name, rows in columns():
        if gen not in name and not (gen == GENS[0] and name == "fan"):
            continue
        assert H.composition(rows) == H.stated_composition(len(rows)), name
        assert [t.kind for t in rows] == [H.COMPOSITION[i % 8] for i in range(len(rows))], name
        assert all(H.kind_of(t.a, t.b, t.c) == t.kind for t in rows), name
        assert all(0.15 < H.along(t) < 0.85 for t in rows), name
    assert len(H.triples(gen)) == H.N_ROWS == 192 and len(H.placed_triples(gen)) == 64 and len(H.fan()) == H.FAN_N


@pytest.mark.parametrize("gen", GENS)
def test_symmetries_keep_every_class(gen):
    for t in H.triples(gen):
        for name, f in H.SYMMETRIES.items():
            u = f(t)  # (asserts on itself)
            assert u.kind == t.kind or name in ("swap a and b", "mirror x", "swap x and y")
    ring = H.polygon_row(H.triples(gen)[0], long=True)[0]
    assert H.rotated(ring, 7)[0] == ring[7] and len(H.rotated(ring, 7)) == len(ring)


@pytest.mark.parametrize("gen", GENS)
def test_far_points_are_certain_and_on_their_side(gen):
    others = lambda t, pts: [p for p in dict.fromkeys(pts) if p not in (t.a, t.b, t.c)]  # noqa: E731
    for t in H.triples(gen) + H.placed_triples(gen):
        r, q, (q2, q1) = H.far_left(t), H.far_right(t), H.far_right_pair(t)
        assert H.exact(t.a, t.b, r) > 0 and all(H.exact(t.a, t.b, p) < 0 for p in (q, q1, q2))
        assert H.exact(t.c, q2, q1) > 0  # the probe triangle is counter-clockwise
        for pts in ([r, q], [r, q1, q2], [p for ring in H.hole_row(t) for p in ring], H.notch_row(t)[0], H.self_line_row(t), [p for m in H.two_lines_row(t) for p in m]):
            assert H.only_planted_is_uncertain(t, others(t, pts)), t
    for t in H.triples(gen)[:16]:  # the long rings: every edge but a -> b is certain about c, and every arc point is left of a -> b
        ring = H.polygon_row(t, long=True)[0]
        assert len(ring) == 48 and len(H.line_row(t, long=True)) == 47 and set(H.line_row(t, long=True)) == set(ring)
        assert all(H.exact(t.a, t.b, p) > 0 for p in ring[2:-1])
        assert all(H.kind_of(s, e, t.c) == H.EASY for s, e in zip(ring[1:-1], ring[2:]))


def test_the_fan_is_a_fan():
    """disjoint polygons: every vertex keeps to the middle of its polygon's own angular sector, between the radii 17 and 61"""
    for ((t, r), (th, w)), poly in zip(zip(H.fan(), H.fan_sectors()), H.fan_polygons()):
        for p in poly[0] + [t.c]:
            ang = np.arctan2(p[1], p[0]) % (2 * np.pi)
            assert th + 0.2 * w < ang < th + 0.8 * w and 17.0 < np.hypot(*p) < 61.0, (t, p)
        assert poly[0][0] == poly[0][-1] == t.a and poly[0][1] == t.b and len(set(poly[0])) == H.FAN_RING - 1
        assert V.validity(V.PG, poly)[0] == V.VALID
        assert all(H.kind_of(s, e, t.c) == H.EASY for s, e in zip(poly[0][1:-1], poly[0][2:]))  # only a -> b is uncertain about c
    n = sum(len(p[0]) for p in H.fan_polygons())
    assert 128 < 2 * np.sqrt(n) <= 256  # build_pip_index: a raster of 256 x 256
    assert len(set(H.fan_points())) == len(H.fan_points()) == 2 * H.FAN_N + 400


# ---- 3. the planted sign decides; the naive twin disagrees ------------------------------------------------------------------------------------


def _f(p):
    return (float(p[0]), float(p[1]))


def naive_points(a, b, c):
    return H.naive(_f(a), _f(b), _f(c))


def naive_arrays(ax, ay, bx, by, cx, cy):
    """exact_predicates.orient's signature: integer arrays on one grid (a power of two times the doubles, so float() is exact for
    every input coordinate; rational sample points are rounded, as a kernel without an exact arm would have them)"""
    f = np.frompyfunc(lambda *v: H.naive((float(v[0]), float(v[1])), (float(v[2]), float(v[3])), (float(v[4]), float(v[5]))), 6, 1)
    return np.asarray(f(ax, ay, bx, by, cx, cy)).astype(np.int64)


_exact_meet = V.meet


def naive_meet(a, b, c, d):
    """validity_ref.meet decides with rational parameters, not with an orientation function; its twin decides WHETHER two segments
    meet the way a kernel does — four orientations, here the signs of the double determinants — and takes the point from the exact
    arithmetic: an end that a zero puts on the other segment, else the crossing of the two lines"""
    o1, o2, o3, o4 = naive_points(a, b, c), naive_points(a, b, d), naive_points(c, d, a), naive_points(c, d, b)
    if o1 == o2 == o3 == o4 == 0:
        return _exact_meet(a, b, c, d)  # collinear segments: nothing planted there
    box = lambda p, s, e: min(s[0], e[0]) <= p[0] <= max(s[0], e[0]) and min(s[1], e[1]) <= p[1] <= max(s[1], e[1])  # noqa: E731
    for p, o, s, e in ((c, o1, a, b), (d, o2, a, b), (a, o3, c, d), (b, o4, c, d)):
        if o == 0 and box(p, s, e):
            return ("point", p)
    if o1 * o2 < 0 and o3 * o4 < 0:
        dx, dy, ex, ey = b[0] - a[0], b[1] - a[1], d[0] - c[0], d[1] - c[1]
        t = ((c[0] - a[0]) * ey - (c[1] - a[1]) * ex) / (dx * ey - dy * ex)
        return ("point", (a[0] + t * dx, a[1] + t * dy))
    return None


def _grid(fn, ka, row_a, kb, row_b):
    a, b = H.on_integer_grid(row_a, row_b)
    return fn(ka, a, kb, b)


def check_tri(kind, row, tris) -> bool:
    try:
        T.check_row(kind, row, np.array(tris))
        return True
    except T.TriangulationError:
        return False


def shell_side(t):
    """+1 when hole_row puts the shell on the left of a -> b"""
    return 1 if -(t.b[1] - t.a[1]) > 0 else -1


# family -> (what to patch: [(module, attribute, twin)], answer(t) over one Triple[, what decides the answer: default the sign])
FAMILIES = {
    "point in polygon": ([(E, "orient", naive_arrays)], lambda t: (E.point_predicate(np.array(t.c), [H.polygon_row(t)], "within"), E.point_predicate(np.array(t.c), [H.polygon_row(t)], "intersects"))),
    "point x line": ([(X, "orient", naive_points)], lambda t: P.mask(P.PT, t.c, P.LS, H.line_row(t))),
    "multipoint x polygon": ([(X, "orient", naive_points)], lambda t: P.mask(P.MPT, H.probe_points(t), P.PG, H.polygon_row(t))),
    "line x line": ([(L, "_orient", naive_points)], lambda t: L.mask_by_rules(L.LS, H.line_row(t), L.LS, H.probe_line(t))),
    "line x polygon": ([(E, "orient", naive_arrays)], lambda t: _grid(R.mask, R.LS, H.probe_line(t), R.PG, H.polygon_row(t))),
    "polygon x polygon": ([(E, "orient", naive_arrays)], lambda t: _grid(Y.mask_by_walks, Y.PG, H.probe_triangle(t), Y.PG, H.polygon_row(t))),
    "validity: a hole vertex": ([(E, "orient", naive_arrays), (V, "meet", naive_meet)], lambda t: V.validity(V.PG, H.hole_row(t))[0],
                                lambda t: t.sign * shell_side(t)),
    "validity: a second member": ([(E, "orient", naive_arrays), (V, "meet", naive_meet)], lambda t: V.validity(V.MPG, H.members_row(t))[0]),
    "is_simple: one line": ([(V, "meet", naive_meet)], lambda t: V.is_simple(V.LS, H.self_line_row(t))),
    "is_simple: two members": ([(V, "meet", naive_meet)], lambda t: V.is_simple(V.MLS, H.two_lines_row(t))),
    # a checker has no answer of its own: it is asked about the triangulation that cuts the ear at c — right only when c is convex
    "triangulation: the ear at c": ([(T, "_orient", naive_points)], lambda t: check_tri(T.PG, H.chain_row(t), [[0, 1, 2], [0, 2, 3]])),
    "triangulation: the ear over c": ([(T, "_orient", naive_points)], lambda t: check_tri(T.PG, H.notch_row(t), [[0, 1, 2], [0, 2, 3], [0, 3, 4]])),
    "hull": ([(X, "orient", naive_points)], lambda t: len(X.exact_hull(H.hull_row(t)))),
}
# W means "wrong or zero": where a reference treats a zero like the true answer (a hull drops a collinear point as it drops an inner
# one, a checker rejects a flat triangle as it rejects a clockwise one) the twin can differ only on the hard rows of the other side —
# half of them.  That is the bar.


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_planted_sign_decides_and_the_naive_twin_disagrees(family, monkeypatch):
    patches, answer = FAMILIES[family][:2]
    key = FAMILIES[family][2] if len(FAMILIES[family]) > 2 else (lambda t: t.sign)
    for gen in GENS:
        rows = H.triples(gen)[:64] + H.placed_triples(gen)[:16]
        exact = [answer(t) for t in rows]
        by_sign = {}
        for t, e in zip(rows, exact):
            if t.kind != H.EASY:  # (an easy row is a tenth of the edge off it: a hole there lies outside altogether)
                by_sign.setdefault(key(t), set()).add(e)
        assert set(by_sign) == {-1, 0, 1} and all(len(v) == 1 for v in by_sign.values()), (family, gen, by_sign)  # the sign alone decides
        assert len({next(iter(v)) for v in by_sign.values()}) >= 2, (family, gen, by_sign)
        with monkeypatch.context() as m:
            for mod, name, twin in patches:
                m.setattr(mod, name, twin)
            twin = [answer(t) for t in rows]
        hard = [i for i, t in enumerate(rows) if t.kind in H.HARD]
        differ = sum(1 for i in hard if twin[i] != exact[i])
        print(f"{family} / {gen}: the naive twin differs on {differ} of {len(hard)} hard rows")
        assert len(hard) == len(rows) // 2
        assert 2 * differ >= len(hard), (family, gen, differ, len(hard))
        if family not in ("line x polygon", "polygon x polygon"):  # (these two classify computed cut points, which the twin sees rounded)
            easy = [i for i, t in enumerate(rows) if t.kind == H.EASY]
            assert all(twin[i] == exact[i] for i in easy)  # the twin is the reference where the filter is certain


def test_second_derivations_agree_on_hard_rows():
    """the twins of two families run on the references' second derivations (mask_by_rules, mask_by_walks): equal to the first here"""
    for gen in GENS:
        for t in H.triples(gen)[:48]:
            assert L.mask_by_rules(L.LS, H.line_row(t), L.LS, H.probe_line(t)) == L.mask(L.LS, H.line_row(t), L.LS, H.probe_line(t))
            assert _grid(Y.mask_by_walks, Y.PG, H.probe_triangle(t), Y.PG, H.polygon_row(t)) == _grid(Y.mask, Y.PG, H.probe_triangle(t), Y.PG, H.polygon_row(t))


def test_integer_grid_is_an_exact_scale():
    from fractions import Fraction

    t = H.triples("mixed")[0]
    a, b = H.on_integer_grid(H.probe_line(t), H.polygon_row(t))
    k = Fraction(a[0][0]) / Fraction(t.c[0])
    assert k.numerator & (k.numerator - 1) == 0 and k.denominator == 1  # a power of two
    assert all(Fraction(i) == Fraction(f) * k for p, q in zip(a, H.probe_line(t)) for i, f in zip(p, q))
    assert all(Fraction(i) == Fraction(f) * k for p, q in zip(b[0], H.polygon_row(t)[0]) for i, f in zip(p, q))


def test_host_triangulation_of_hard_rows(drivers):
    """tri::orient's expansion arm on the host (tests/triangulate_host_driver.cpp, plain and under AddressSanitizer + UBSan): c as a
    vertex between a and b, c beside the diagonal of an ear, c as the hole vertex the bridge starts from — every valid row status 0 and
    through the checker; tests/test_gpu_hard_orient.py holds the device to the same indices"""
    from tests.test_triangulate_host import check, run

    built, workdir = drivers
    for gen in GENS:
        ts = H.triples(gen)[:64]
        rows = [f(t) for t in ts for f in (H.chain_row, H.notch_row, H.hole_row)] + [H.hole_row(t, True) for t in ts[:24]]
        codes = V.validity_column(V.PG, rows)[0]
        assert all(codes[3 * i] == codes[3 * i + 1] == V.VALID for i in range(len(ts)))  # (chain and notch rows are valid whatever the sign)
        plain = run(built["plain"], workdir, V.PG, rows)
        assert check(V.PG, rows, None, codes, plain) == int((codes == V.VALID).sum()) >= len(rows) * 3 // 4
        san = run(built["sanitized"], workdir, V.PG, rows)
        assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(plain, san))
        for i, t in enumerate(ts):  # what the planted sign forces: the ear at c exists only when c is convex, the ear over c only when c is left
            cut_at_c = any(sorted(tri) == [0, 1, 2] for tri in plain[3 * i][1].tolist())
            cut_over_c = any(sorted(tri) == [0, 1, 2] for tri in plain[3 * i + 1][1].tolist())
            assert (not cut_at_c or t.sign < 0) and (not cut_over_c or t.sign > 0), (gen, i, t)


from tests.test_triangulate_host import drivers  # noqa: E402,F401  (the fixture that builds the two host drivers)


# ---- 5. the figures for the constructive kernels (tests/hard_clip.py; the GPU side is tests/test_gpu_hard_clip.py) ---------------------------------
#
# A "shape" is (status, (parts, rings, coordinates per ring with the closing one), which input coordinate or crossing stands where).


def by_sign(ts, shapes):
    """{exact sign of the planted triple: the set of shapes its rows have}, easy rows included"""
    out = {}
    for t, s in zip(ts, shapes):
        out.setdefault(t.sign, set()).add(s)
    return out


def assert_column(ts, n_rows):
    """the column keeps COMPOSITION (classified anew, without the collinear rows where the figure has none) and at least 96 rows are hard"""
    want = H.stated_composition(H.N_ROWS)
    if n_rows != H.N_ROWS:
        assert n_rows == H.N_ROWS - want[H.COLLINEAR] == 168 and want[H.COLLINEAR] == 24
        want = {k: v for k, v in want.items() if k != H.COLLINEAR}
    assert len(ts) == n_rows and H.composition(ts) == want
    assert [t.kind for t in ts] == [k for i in range(H.N_ROWS) for k in [H.COMPOSITION[i % 8]] if n_rows == H.N_ROWS or k != H.COLLINEAR]
    assert sum(1 for t in ts if t.kind in H.HARD and H.classes(t.a, t.b, t.c) == "WWWWWW") >= 96


def assert_only_planted_is_uncertain(t, rings_a, rings_b):
    planted = {t.a, t.b, t.c}
    for s, e, p in K.edge_vertex_evaluations(rings_a, rings_b):
        if {s, e, p} != planted:
            assert K.certain_and_off(s, e, p), (t, s, e, p)


# figure -> form -> operation -> {sign: (parts, rings, coordinates per ring)}, stated by hand from the figures' docstrings
COUNTS = {
    ("pass", "short"): {"A&B": {1: (1, 1, (5,)), 0: (1, 1, (4,)), -1: (1, 1, (4,))}, "B&A": {1: (1, 1, (5,)), 0: (1, 1, (4,)), -1: (1, 1, (4,))},
                        "A-B": {1: (1, 1, (8,)), 0: (1, 1, (7,)), -1: (1, 1, (7,))}, "B-A": {1: (1, 1, (5,)), 0: (1, 1, (5,)), -1: (1, 1, (6,))},
                        "A|B": {1: (1, 1, (8,)), 0: (1, 1, (8,)), -1: (1, 1, (9,))}, "B|A": {1: (1, 1, (8,)), 0: (1, 1, (8,)), -1: (1, 1, (9,))}},
    # the long ring has 44 more coordinates; they are all outside B
    ("pass", "long"): {"A&B": {1: (1, 1, (5,)), 0: (1, 1, (4,)), -1: (1, 1, (4,))}, "B&A": {1: (1, 1, (5,)), 0: (1, 1, (4,)), -1: (1, 1, (4,))},
                       "A-B": {1: (1, 1, (52,)), 0: (1, 1, (51,)), -1: (1, 1, (51,))}, "B-A": {1: (1, 1, (5,)), 0: (1, 1, (5,)), -1: (1, 1, (6,))},
                       "A|B": {1: (1, 1, (52,)), 0: (1, 1, (52,)), -1: (1, 1, (53,))}, "B|A": {1: (1, 1, (52,)), 0: (1, 1, (52,)), -1: (1, 1, (53,))}},
    # a far triangle is the first member of either row: one more part wherever its row is kept
    ("pass", "multi"): {"A&B": {1: (1, 1, (5,)), 0: (1, 1, (4,)), -1: (1, 1, (4,))}, "B&A": {1: (1, 1, (5,)), 0: (1, 1, (4,)), -1: (1, 1, (4,))},
                        "A-B": {1: (2, 2, (4, 8)), 0: (2, 2, (4, 7)), -1: (2, 2, (4, 7))}, "B-A": {1: (2, 2, (4, 5)), 0: (2, 2, (4, 5)), -1: (2, 2, (4, 6))},
                        "A|B": {1: (3, 3, (4, 8, 4)), 0: (3, 3, (4, 8, 4)), -1: (3, 3, (4, 9, 4))}, "B|A": {1: (3, 3, (4, 8, 4)), 0: (3, 3, (4, 8, 4)), -1: (3, 3, (4, 9, 4))}},
    # the box holds the ring: the same counts for either sign — the sign shows in the ORDER of the coordinates (below)
    ("spike", "short"): {op: {1: c, -1: c} for op, c in {"A&B": (1, 1, (5,)), "B&A": (1, 1, (5,)), "A-B": (0, 0, ()), "B-A": (1, 2, (5, 5))}.items()},
    ("nested", "short"): {op: {1: c, -1: c} for op, c in {"A&B": (1, 2, (4, 4)), "B&A": (1, 2, (4, 4)), "A-B": (0, 0, ()), "B-A": (2, 3, (5, 4, 4))}.items()},
    ("hinge", "short"): {"A&B": {1: (1, 1, (4,)), 0: (0, 0, ()), -1: (0, 0, ())}, "B&A": {1: (1, 1, (4,)), 0: (0, 0, ()), -1: (0, 0, ())},
                         "A-B": {1: (1, 1, (6,)), 0: (1, 1, (4,)), -1: (1, 1, (4,))}, "B-A": {1: (1, 1, (4,)), 0: (1, 1, (4,)), -1: (1, 1, (4,))},
                         "A|B": {1: (1, 1, (6,)), 0: (1, 1, (6,)), -1: (2, 2, (4, 4))}, "B|A": {1: (1, 1, (6,)), 0: (1, 1, (6,)), -1: (2, 2, (4, 4))}},
}
FIGURE_FORMS = [(f, form) for f in K.FORMS for form in K.FORMS[f]]


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("figure,form", FIGURE_FORMS, ids=[f"{f}-{form}" for f, form in FIGURE_FORMS])
def test_clip_figures(figure, form, gen):
    """what tests/test_gpu_hard_clip.py relies on, on the references alone: the column keeps COMPOSITION (the spike and the nested hole
    without their 24 collinear rows, which are invalid polygons; nothing else is left out) and at least 96 rows are hard; only the
    planted triple is uncertain among all (edge, vertex) evaluations of the two rows; the transitions of every segment are MIN_GAP
    apart by the headers' own definition; every operation has status 0 or 2 and ONE shape per exact sign, stated above as counts; and
    for intersection, difference and union the shapes of + and - differ in at least one operand order — a kernel that follows the sign
    of the double determinant, wrong on the 96 hard rows, returns the other sign's shape there.  The nested hole is the exception:
    its hole is inside its shell whatever the sign (that is what makes the row valid), so both signs have one shape, and the power
    comes from the question itself: the crossing number of c against the shell with the double sign says `outside` on every hard row."""
    ts, ka, A, kb, B = K.poly_rows(figure, gen, form)
    assert_column(ts, 168 if figure in K.DROPS_COLLINEAR else 192)
    for t, a, b in list(zip(ts, A, B))[: 16 if form == "long" else len(ts)]:  # (the arc of the long ring is one construction: a sample, as below)
        assert_only_planted_is_uncertain(t, K.flat_rings(ka, a), K.flat_rings(kb, b))
    differ = {}
    for op in K.OPS_OF[figure]:
        name = K.POLY_OPS[op][3]
        got = K.poly_expected(figure, gen, form, op)
        assert all(r.status in (C.ST_OK, C.ST_EMPTY) for r in got), (figure, form, gen, op)
        gaps = K.poly_gaps(figure, gen, form, op)
        assert all(g is None or g >= C.MIN_GAP for g in gaps), (figure, form, gen, op, min(g for g in gaps if g is not None))
        shapes = by_sign(ts, [r.shape() for r in got])
        assert all(len(v) == 1 for v in shapes.values()), (figure, form, gen, op, {s: len(v) for s, v in shapes.items()})
        assert {s: next(iter(v))[1] for s, v in shapes.items()} == COUNTS[figure, form][op], (figure, form, gen, op)
        differ[name] = differ.get(name, False) or shapes[1] != shapes[-1]
    if figure == "nested":
        assert not any(differ.values())
        hard = [(t, a) for t, a in zip(ts, A) if t.kind in H.HARD]
        assert len(hard) == 96 and all(naive_crossing_number(t.c, a[0]) <= 0 < C.ring_position(*H.on_integer_grid(t.c, a[0])) for t, a in hard)
    else:
        assert differ == {K.POLY_OPS[op][3]: True for op in K.OPS_OF[figure]}, (figure, form, gen, differ)


def naive_crossing_number(pt, ring):
    """polyclip_ref.ring_position with the sign of the double determinant in place of the exact cross product"""
    inside = False
    for a, b in zip(ring, ring[1:]):
        s = H.naive(a, b, pt)
        if s == 0 and min(a[0], b[0]) <= pt[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= pt[1] <= max(a[1], b[1]):
            return 0
        if (a[1] > pt[1]) != (b[1] > pt[1]) and (b[1] > a[1]) == (s > 0):
            inside = not inside
    return 1 if inside else -1


def test_spike_ring_turns_at_its_apex():
    """the placement the spike ring needs, asserted with seqedit_ref and not assumed: the lexicographically smallest coordinate is the
    apex a (index 0), its neighbours are b and c, so the turn gpk_orient_polygons takes is orient(b, a, c) — the planted triple —, on
    the short ring and on the one of more than SHORT_RING coordinates; the exact shoelace sign (Fractions) is that turn's sign; and the
    sign of the f64 shoelace sum, or of the double determinant, is wrong on every hard row"""
    from tests import seqedit_ref as S

    with open(os.path.join(H.CSRC, "gpk_seqedit.hip")) as f:
        assert "constexpr int SHORT_RING = 256;" in f.read() and H.LONG_ARC + 5 > 256
    for gen in GENS:
        n_hard = 0
        for t0 in H.triples(gen):
            for long in (False, True):
                t = H.spike_triple(t0, long)
                ring = np.array(H.spike_row(t0, long)[0])
                assert len(ring) == (H.LONG_ARC + 5 if long else 5) and t.kind == t0.kind and t.sign == t0.sign
                s, v, u, w = S.ring_turn(ring)
                assert (v, u, w) == (0, len(ring) - 2, 1) and tuple(ring[u]) == t.b and tuple(ring[v]) == t.a and tuple(ring[w]) == t.c
                assert s == H.exact(t.b, t.a, t.c) == -t.sign
                f = [(Fraction(float(x)), Fraction(float(y))) for x, y in ring]
                area2 = sum(f[i][0] * f[i + 1][1] - f[i + 1][0] * f[i][1] for i in range(len(f) - 1))
                assert (area2 > 0) - (area2 < 0) == s if t.kind != H.COLLINEAR else s == 0 != area2  # (a collinear row touches itself: s == 0, whatever its area)
                if t.kind in H.HARD:
                    assert H.naive(t.b, t.a, t.c) != s
                    n_hard += not long
        assert n_hard == 96


LINE_SHAPES = {  # mode -> sign -> parts as ((tag, number of the coordinate) or "x" for a crossing): the line is [w, c, q1]
    LC.INSIDE: {1: (((LC.TAG_L, 0), (LC.TAG_L, 1), "x"),), 0: (((LC.TAG_L, 0), (LC.TAG_L, 1)),), -1: (((LC.TAG_L, 0), "x"),)},
    LC.OUTSIDE: {1: (("x", (LC.TAG_L, 2)),), 0: (((LC.TAG_L, 1), (LC.TAG_L, 2)),), -1: (("x", (LC.TAG_L, 1), (LC.TAG_L, 2)),)},
}


@pytest.mark.parametrize("long", [False, True], ids=["short", "long"])
@pytest.mark.parametrize("gen", GENS)
def test_line_clip_figure(gen, long):
    """the line [w, c, q1] of the pass figure against A, for the four families: all 192 rows, the transitions apart, one shape per
    exact sign — stated above; a MULTILINESTRING numbers its coordinates after the two of its far member, whose one part comes first
    in the outside —, three different shapes in either mode"""
    for kl, kp in K.LINE_FAMILIES:
        ts, lines, polys = K.line_rows(gen, kl, kp, long)
        assert_column(ts, 192)
        if (kl, kp) == (LC.MLS, LC.MPG) or not long:
            for t, l, p in zip(ts[: 16 if long else 192], lines, polys):
                assert_only_planted_is_uncertain(t, K.flat_rings(kl, l), K.flat_rings(kp, p))
        for mode in (LC.INSIDE, LC.OUTSIDE):
            got = K.line_expected(gen, kl, kp, long, mode)
            gaps = K.line_gaps(gen, kl, kp, long, mode)
            assert all(g is None or g >= LC.MIN_GAP for g in gaps), (gen, kl, kp, mode)
            shapes = by_sign(ts, [r.shape() for r in got])
            assert all(len(v) == 1 for v in shapes.values())
            k0 = 2 if kl == LC.MLS else 0
            want = {s: tuple(tuple(e if e == "x" else (e[0], e[1] + k0) for e in pt) for pt in parts) for s, parts in LINE_SHAPES[mode].items()}
            if kl == LC.MLS and mode == LC.OUTSIDE:
                want = {s: (((LC.TAG_L, 0), (LC.TAG_L, 1)),) + parts for s, parts in want.items()}
            assert {s: next(iter(v)) for s, v in shapes.items()} == want, (gen, kl, kp, mode)
            assert len({next(iter(v)) for v in shapes.values()}) == 3


def test_transition_gap_is_the_headers_definition():
    """transition_gap counts points where kept-ness changes, a segment's own ends included when they are such points, and nothing else:
    on the hand cases it is never above the references' own figures where both exist for a segment's inner cuts, it is None for a
    ring kept whole, and on the pass figure it is the 0.04 .. 0.07 between c and the crossing of q2 -> w on A's edge while `clip`'s third value
    — every cut of a segment, its ends included — is the 1e-17 between c and the crossing next to it"""
    assert C.transition_gap(C.PG, [C.S10], C.PG, [C.sq(2, 2, 5, 5)], C.INTERSECTION) is None  # b inside a: no transition at all
    assert C.transition_gap(C.PG, [C.S10], C.PG, [C.sq(5, 5, 15, 15)], C.INTERSECTION) is None  # one crossing an edge; the corner (10, 10) is kept on both hands
    for mode in (C.INTERSECTION, C.DIFFERENCE):  # a bar across: both upright edges of the square are crossed at 4 and at 6 of 10
        assert C.transition_gap(C.PG, [C.S10], C.PG, [C.sq(-2, 4, 12, 6)], mode) == Fraction(1, 5)
    assert U.transition_gap(U.PG, [U.S10], U.PG, [U.sq(-2, 4, 12, 6)]) == Fraction(1, 5)
    assert LC.transition_gap(LC.LS, [(-2, 5), (12, 5)], LC.PG, [C.S10], LC.INSIDE) == Fraction(10, 14)
    assert LC.transition_gap(LC.LS, [(-3, 5), (0, 5), (4, 5)], LC.PG, [C.S10], LC.INSIDE) is None  # one transition, at the vertex (0, 5)
    assert LC.transition_gap(LC.LS, [(-3, 5), (0, 5), (12, 5)], LC.PG, [C.S10], LC.INSIDE) == Fraction(10, 12)  # the vertex and the exit
    t = next(t for t in H.triples("mixed") if t.kind == H.HARD_LEFT)
    a, b = H.on_integer_grid(*H.pass_rows(t)[:2])
    every_cut = C.clip(C.PG, a, C.PG, b, C.INTERSECTION)[2]
    gap = C.transition_gap(C.PG, a, C.PG, b, C.INTERSECTION)
    assert every_cut < Fraction(1, 10**12) and Fraction(1, 30) < gap < Fraction(1, 10)


# ---- 4. census of the earlier fixtures ----------------------------------------------------------------------------------------------------------


def pair_evaluations(seqs_a, seqs_b, boxed=False):
    """every (segment start, segment end, vertex) of a segment of one side and a vertex of the other: what a segment-against-segment
    test asks.  boxed: only a vertex in the closed box of the segment, what coord_pos_relative_to_ring asks about a point"""
    for own, other in ((seqs_a, seqs_b), (seqs_b, seqs_a)):
        pts = [tuple(map(float, p)) for s in other for p in s]
        for s in own:
            ring = [tuple(map(float, p)) for p in s]
            if boxed:
                yield from H.ring_evaluations(ring, pts)
            else:
                yield from ((a, b, p) for a, b in zip(ring[:-1], ring[1:]) if a != b for p in pts)


def fast_census(evaluations):
    """hard_orient.census with the rational sign taken only where the filter is uncertain (a certain evaluation is F, or Z when both
    products are zero: what test_replica_against_the_rational_sign holds the filter to)"""
    out = {"n": 0, "Z": 0, "F": 0, "U": 0, "W": 0}
    for a, b, c in evaluations:
        out["n"] += 1
        certain, d = H.stage_a(a, b, c)
        out[("Z" if d == 0 else "F") if certain else H.classify(a, b, c)] += 1
    return out


def earlier_fixtures():
    geoms = X.buildings(150, seed=11) + X.dyadic_buildings(120)
    pts, rows = X.probe_points(geoms)
    yield "test_gpu_georeferenced: probe_points on buildings", (ev for p, r in zip(pts, rows) for poly in geoms[r] for ev in pair_evaluations(poly, [[p]], boxed=True))
    geoms = X.buildings(60, seed=12, holes=False, multi=False) + X.dyadic_buildings(40, seed=13)
    lines = [g[0][0] for g in geoms]
    pts, rows = X.probe_points([[[l]] for l in lines] * 2, seed=14)
    yield "test_gpu_georeferenced: probe_points on linestrings", (ev for p, r in zip(pts, rows % len(lines)) for ev in pair_evaluations([lines[r]], [[p]], boxed=True))
    from tests.lattice import concentric_pair, nudged, random_pair

    rng = random.Random(21)
    pairs = []
    for _ in range(6000):
        pa, pb = concentric_pair(rng) if rng.random() < 0.6 else random_pair(rng)
        pairs.append((nudged(pa, rng), nudged(pb, rng)))
    close = lambda poly: [list(r) + ([r[0]] if r[0] != r[-1] else []) for r in poly]  # noqa: E731
    yield "test_gpu_contains: the first 1500 nudged pairs", (ev for pa, pb in pairs[:1500] for ev in pair_evaluations(close(pa), close(pb)))
    rng = np.random.default_rng(77)
    sliver = []
    for k in range(256):
        x0 = float(rng.uniform(0.1, 0.9))
        eps = float(np.spacing(x0) * int(rng.integers(1, 5)))
        ring = [(-1.0, -2.0), (2.0, -2.0), (2.0, -1.0), (x0 + eps, -1.0), (x0, 1.0), (x0 - eps, -1.0), (-1.0, -1.0), (-1.0, -2.0)]
        sliver.append(([[(0.0, 0.0), (1.0, 0.0)]], [ring]))
    yield "test_gpu_lineclip: the sliver rows", (ev for a, b in sliver for ev in pair_evaluations(a, b))
    e = 2.0**-40
    a = (1.0 + e, 1.0 + 3 * e)
    b = (a[0] + 12.0 + 3 * e, a[1] + 4.0 + e)
    mid = (a[0] + 6.0 + 1.5 * e, a[1] + 2.0 + 0.5 * e)
    shell = [a, b, (13.0, 30.0), (1.0, 30.0), a]
    three = []
    for dy in (0.0, np.nextafter(mid[1], np.inf) - mid[1], np.nextafter(mid[1], -np.inf) - mid[1]):
        v = (mid[0], mid[1] + dy)
        three.append(([shell], [[v, (6.0, 12.0), (8.0, 12.0), v]]))
    yield "test_gpu_validity: the three slope-1/3 rows", (ev for s, h in three for ev in pair_evaluations(s, h))
    for gen in GENS:
        yield f"hard_orient.triples({gen}): the planted evaluations, all six orders", ((t[i], t[j], t[k]) for t in H.triples(gen) for i, j, k in H.ORDERS)


def test_census_of_earlier_fixtures(capsys):
    """reported, not asserted (only that the new columns hold what they say): evaluations (segment start, segment end, vertex) — for
    point probes the edges whose closed box holds the point, for pairs of rows every segment of one against every vertex of the other"""
    lines = ["fixture | evaluations | Z | F | U | W"]
    got = {}
    for name, evs in earlier_fixtures():
        c = fast_census(evs)
        got[name] = c
        lines.append(f"{name} | {c['n']} | {c['Z']} | {c['F']} | {c['U']} | {c['W']}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for gen in GENS:
        c = got[f"hard_orient.triples({gen}): the planted evaluations, all six orders"]
        assert c["W"] == 96 * 6 and c["U"] == 48 * 6 and c["Z"] == 24 * 6 and c["F"] == 24 * 6
