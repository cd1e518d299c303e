"""The figures of tests/hard_orient.py for the constructive kernels as columns, with their exact results: shared by
tests/test_hard_orient.py (no GPU: what the figures promise) and tests/test_gpu_hard_clip.py (GPU: gpk_line_clip, gpk_polygon_clip,
gpk_polygon_union, gpk_intersection_measure, gpk_orient_polygons on them).

Every pair of rows is brought to its own integer grid (hard_orient.on_integer_grid: one exact power of two), run through the exact
references there (polyclip_ref.clip, polyunion_ref.union, lineclip_ref.clip), and scaled back: input coordinates come back as the
doubles they were, crossings as Fractions.  Results are computed once per (figure, generator, form, operation) and kept."""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

from tests import hard_orient as H
from tests import lineclip_ref as LC
from tests import polyclip_ref as C
from tests import polyunion_ref as U

LS, MLS, PG, MPG = LC.LS, LC.MLS, C.PG, C.MPG
GENS = sorted(H.GENERATORS)
# operation -> (reference, mode, operands swapped, the library's name of the operation)
POLY_OPS = {"A&B": (C.clip, C.INTERSECTION, False, "intersection"), "B&A": (C.clip, C.INTERSECTION, True, "intersection"),
            "A-B": (C.clip, C.DIFFERENCE, False, "difference"), "B-A": (C.clip, C.DIFFERENCE, True, "difference"),
            "A|B": (U.union, U.UNION, False, "union"), "B|A": (U.union, U.UNION, True, "union")}
POLY_GAPS = {"intersection": C.transition_gap, "difference": C.transition_gap, "union": U.transition_gap}
FORMS = {"pass": ("short", "long", "multi"), "spike": ("short",), "nested": ("short",), "hinge": ("short",)}
CLIP_OPS = ("A&B", "B&A", "A-B", "B-A")
OPS_OF = {"pass": tuple(POLY_OPS), "hinge": tuple(POLY_OPS), "spike": CLIP_OPS, "nested": CLIP_OPS}  # (a box united with what it holds is the box)
DROPS_COLLINEAR = ("spike", "nested")  # a collinear row of these is an invalid polygon (a ring that touches itself, a hole on its shell)


@lru_cache(maxsize=None)
def poly_rows(figure: str, gen: str, form: str = "short"):
    """(triples, kind of A, rows of A, kind of B, rows of B): the triples are the ones the rows are built around (turned, for the spike
    and the nested hole), in the column's order; the 24 collinear rows are left out of DROPS_COLLINEAR figures and of nothing else"""
    assert form in FORMS[figure]
    ts = [t for t in H.triples(gen) if not (figure in DROPS_COLLINEAR and t.kind == H.COLLINEAR)]
    if figure == "pass":
        kind = MPG if form == "multi" else PG
        rows = [H.pass_rows(t, form == "long", form == "multi") for t in ts]
        return tuple(ts), kind, [r[0] for r in rows], kind, [r[1] for r in rows]
    if figure == "spike":
        A = [H.spike_row(t) for t in ts]
        return tuple(H.spike_triple(t) for t in ts), PG, A, PG, [H.box_around(a) for a in A]
    if figure == "nested":
        A = [H.nested_row(t) for t in ts]
        return tuple(H.nested_triple(t) for t in ts), PG, A, PG, [H.box_around(a) for a in A]
    assert figure == "hinge"
    rows = [H.hinge_rows(t) for t in ts]
    return tuple(ts), PG, [r[0] for r in rows], PG, [r[1] for r in rows]


class PolyResult(NamedTuple):
    parts: object  # on the integer grid, as the reference returns them
    status: int
    ka: int
    a: object  # the first operand on the integer grid
    kb: int
    b: object
    scale: int

    def scaled_back(self):
        return C.scaled_back(self.parts, self.ka, self.a, self.kb, self.b, self.scale)

    def shape(self):
        return self.status, C.counts_of(self.parts), C.shape_of(self.parts, self.ka, self.a, self.kb, self.b)


@lru_cache(maxsize=None)
def poly_expected(figure: str, gen: str, form: str, op: str):
    """[PolyResult] of one operation over the rows of poly_rows"""
    fn, mode, swapped, _name = POLY_OPS[op]
    _ts, ka, A, kb, B = poly_rows(figure, gen, form)
    if swapped:
        ka, A, kb, B = kb, B, ka, A
    out = []
    for a, b in zip(A, B):
        ia, ib = H.on_integer_grid(a, b)
        parts, status, _gap = fn(ka, ia, kb, ib, mode)
        out.append(PolyResult(parts, status, ka, ia, kb, ib, H.integer_grid_scale(a, b)))
    return out


def poly_gaps(figure: str, gen: str, form: str, op: str):
    """transition_gap of every row of one operation"""
    _fn, mode, _swapped, name = POLY_OPS[op]
    return [POLY_GAPS[name](r.ka, r.a, r.kb, r.b, mode) for r in poly_expected(figure, gen, form, op)]


# ---- the line of the pass figure against A -------------------------------------------------------------------------------------------------

LINE_FAMILIES = [(LS, PG), (LS, MPG), (MLS, PG), (MLS, MPG)]


@lru_cache(maxsize=None)
def line_rows(gen: str, kl: int, kp: int, long: bool = False):
    """(triples, line rows, polygon rows) of the pass figure: [w, c, q1] against (a, b, r); a MULTI row has the figure as its second member"""
    ts = H.triples(gen)
    lines = [H.pass_rows(t, long, kl == MLS)[2] for t in ts]
    polys = [H.pass_rows(t, long, kp == MPG)[0] for t in ts]
    return ts, lines, polys


class LineResult(NamedTuple):
    result: object  # (parts, crossings, min gap) on the integer grid
    line: object
    poly: object
    scale: int

    def scaled_back(self):
        return LC.scaled_back(self.result, self.scale)

    def shape(self):
        return tuple(tuple("x" if tag == LC.TAG_X else (tag, k) for tag, k in pt) for pt in self.result[0])


@lru_cache(maxsize=None)
def line_expected(gen: str, kl: int, kp: int, long: bool, mode: int):
    _ts, lines, polys = line_rows(gen, kl, kp, long)
    out = []
    for l, p in zip(lines, polys):
        il, ip = H.on_integer_grid(l, p)
        out.append(LineResult(LC.clip(kl, il, kp, ip, mode), il, ip, H.integer_grid_scale(l, p)))
    return out


def line_gaps(gen: str, kl: int, kp: int, long: bool, mode: int):
    return [LC.transition_gap(kl, r.line, kp, r.poly, mode) for r in line_expected(gen, kl, kp, long, mode)]


# ---- what a figure's rows are made of, for the "only the planted triple is uncertain" assertion ---------------------------------------------


def certain_and_off(a, b, c) -> bool:
    """EASY without the rational sign: certain under all six orders, the double determinant not zero (a certified sign is the exact
    one: tests/test_hard_orient.py::test_replica_against_the_rational_sign)"""
    t = (a, b, c)
    for i, j, k in H.ORDERS:
        certain, d = H.stage_a(t[i], t[j], t[k])
        if not certain or d == 0:
            return False
    return True


def edge_vertex_evaluations(rings_a, rings_b):
    """every (edge start, edge end, vertex) a clip can ask about: an edge of one row against a vertex of the other, and an edge of a
    row against a vertex of the same row that is not one of its ends (ring signs, turns, junctions)"""
    for own, other in ((rings_a, rings_b), (rings_b, rings_a)):
        pts = list(dict.fromkeys(p for r in other for p in r))
        for r in own:
            for s, e in zip(r[:-1], r[1:]):
                for p in pts + [q for q in dict.fromkeys(r) if q not in (s, e)]:
                    if p not in (s, e):
                        yield s, e, p


def flat_rings(kind, row):
    """the coordinate sequences of a row of any of the four kinds"""
    if kind == LS:
        return [row]
    if kind in (MLS, PG):
        return list(row)
    return [r for p in row for r in p]
