"""Exact reference of the row-wise distance between two non-point geometries (gpk_distance_rowwise, csrc/gpk_pairdist.hip).

Rows are described as in exact_ref (kind, row): a MULTIPOINT's list of points, a LINESTRING's coordinates, a MULTILINESTRING's
linestrings, a POLYGON's closed rings (exterior first), a MULTIPOLYGON's polygons.  The contract:
  * an empty row (no member has a coordinate) on either side: None (NaN on the GPU);
  * 0 exactly when the closed point sets intersect: a segment of one side meets a segment of the other, or a vertex of one side is
    inside or on a polygonal other side (holes excluded);
  * otherwise the minimum, over every vertex of one side and every segment of the other (both ways), of the exact point-segment
    distance.  A one-coordinate sequence and every MULTIPOINT member is a degenerate segment; every ring counts.
Near-minimal pairs are found with f64 first and evaluated exactly in Fractions; the segment crossing test is exact wherever the f64
orientation is not certain."""
from fractions import Fraction

import numpy as np

from tests import exact_ref as X

POLYGONAL = X.POLYGONAL


def is_empty(kind: int, row) -> bool:
    return sum(len(s) for s in X.row_seqs(kind, row)) == 0


def segments(kind: int, row):
    """(starts, ends) f64 arrays: one segment per coordinate, (c, c + 1) inside a sequence, else degenerate (c, c)"""
    s0, s1 = [], []
    for s in X.row_seqs(kind, row):
        s = np.asarray(s, dtype=np.float64).reshape(-1, 2)
        if len(s) == 0:
            continue
        s0.append(s)
        s1.append(np.concatenate([s[1:], s[-1:]]))
    return np.concatenate(s0), np.concatenate(s1)


def lmax(kind: int, row) -> float:
    a, b = segments(kind, row)
    return float(np.max(np.hypot(*(b - a).T))) if len(a) else 0.0


def segments_intersect(a0, a1, b0, b1) -> bool:
    """closed segments (possibly degenerate) share a point — exact"""
    a0, a1, b0, b1 = [tuple(map(float, p)) for p in (a0, a1, b0, b1)]
    if a0 == a1:
        return X.on_segment(a0, b0, b1)
    if b0 == b1:
        return X.on_segment(b0, a0, a1)
    o1, o2 = X.orient(a0, a1, b0), X.orient(a0, a1, b1)
    o3, o4 = X.orient(b0, b1, a0), X.orient(b0, b1, a1)
    if o1 != o2 and o3 != o4 and o1 * o2 <= 0 and o3 * o4 <= 0:
        return True
    return X.on_segment(b0, a0, a1) or X.on_segment(b1, a0, a1) or X.on_segment(a0, b0, b1) or X.on_segment(a1, b0, b1)


def _orient_f64(a, b, c):
    """vectorised orientation sign and whether f64 certifies it"""
    l = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1])
    r = (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    d = l - r
    sure = np.abs(d) > 1e-12 * (np.abs(l) + np.abs(r))
    return np.sign(d), sure


def _crossing_candidates(a0, a1, b0, b1):
    """indices (i, j) of segment pairs that are not certainly disjoint (box overlap and no certain separating orientation)"""
    out = []
    step = max(1, 2_000_000 // max(len(b0), 1))
    blx, bhx = np.minimum(b0[:, 0], b1[:, 0]), np.maximum(b0[:, 0], b1[:, 0])
    bly, bhy = np.minimum(b0[:, 1], b1[:, 1]), np.maximum(b0[:, 1], b1[:, 1])
    for i0 in range(0, len(a0), step):
        p0, p1 = a0[i0:i0 + step], a1[i0:i0 + step]
        box = ((np.maximum(p0[:, 0], p1[:, 0])[:, None] >= blx) & (np.minimum(p0[:, 0], p1[:, 0])[:, None] <= bhx)
               & (np.maximum(p0[:, 1], p1[:, 1])[:, None] >= bly) & (np.minimum(p0[:, 1], p1[:, 1])[:, None] <= bhy))
        ii, jj = np.nonzero(box)
        if len(ii) == 0:
            continue
        P0, P1, Q0, Q1 = p0[ii], p1[ii], b0[jj], b1[jj]
        s1, c1 = _orient_f64(P0, P1, Q0)
        s2, c2 = _orient_f64(P0, P1, Q1)
        s3, c3 = _orient_f64(Q0, Q1, P0)
        s4, c4 = _orient_f64(Q0, Q1, P1)
        apart = (c1 & c2 & (s1 == s2) & (s1 != 0)) | (c3 & c4 & (s3 == s4) & (s3 != 0))
        keep = ~apart
        out += list(zip((ii[keep] + i0).tolist(), jj[keep].tolist()))
    return out


def _test_vertices(kind: int, row):
    """one vertex per non-empty sequence (every point of a MULTIPOINT)"""
    return [s[0] for s in X.row_seqs(kind, row) if len(s)]


def intersects(ka: int, ra, kb: int, rb) -> bool:
    """closed point sets of two non-empty rows intersect (exact).  Rings are taken to be closed, as every fixture's are."""
    if kb in POLYGONAL:
        polys = X.row_polys(kb, rb)
        if any(X.geom_position(v, polys) >= 0 for v in _test_vertices(ka, ra)):
            return True
    if ka in POLYGONAL:
        polys = X.row_polys(ka, ra)
        if any(X.geom_position(v, polys) >= 0 for v in _test_vertices(kb, rb)):
            return True
    a0, a1 = segments(ka, ra)
    b0, b1 = segments(kb, rb)
    return any(segments_intersect(a0[i], a1[i], b0[j], b1[j]) for i, j in _crossing_candidates(a0, a1, b0, b1))


def _vertex_segment_f64(p, a, b, cut=None):
    """f64 distances of every vertex p[i] to every segment (a[j], b[j]), in chunks: their minimum, or (cut given) the pairs
    (i, j) within `cut`"""
    d = b - a
    d2 = np.sum(d * d, axis=1)
    step = max(1, 1_000_000 // max(len(a), 1))
    best, pairs = np.inf, []
    for i0 in range(0, len(p), step):
        q = p[i0:i0 + step]
        t = ((q[:, None, 0] - a[:, 0]) * d[:, 0] + (q[:, None, 1] - a[:, 1]) * d[:, 1]) / np.where(d2 > 0, d2, 1.0)
        t = np.clip(t, 0.0, 1.0)
        dist = np.hypot(a[:, 0] + t * d[:, 0] - q[:, None, 0], a[:, 1] + t * d[:, 1] - q[:, None, 1])
        if cut is None:
            best = min(best, float(dist.min()))
        else:
            ii, jj = np.nonzero(dist <= cut)
            pairs += list(zip((ii + i0).tolist(), jj.tolist()))
    return best if cut is None else pairs


def distance2(ka: int, ra, kb: int, rb):
    """exact squared set distance (Fraction) of two non-empty rows"""
    if intersects(ka, ra, kb, rb):
        return Fraction(0)
    a0, a1 = segments(ka, ra)
    b0, b1 = segments(kb, rb)
    scale = float(max(np.max(np.abs(a0)), np.max(np.abs(b0)), 1e-300))
    best_f = min(_vertex_segment_f64(a0, b0, b1), _vertex_segment_f64(b0, a0, a1))
    cut = best_f * (1 + 1e-6) + 1e-12 * scale
    best = None
    for p, s, e in ((a0, b0, b1), (b0, a0, a1)):
        for i, j in _vertex_segment_f64(p, s, e, cut):
            d = X.point_segment_dist2(p[i], s[j], e[j])
            best = d if best is None or d < best else best
    return best


def distance(ka: int, ra, kb: int, rb):
    """(Decimal exact distance or None for an empty side, a-priori bound of the f64 evaluation)"""
    if is_empty(ka, ra) or is_empty(kb, rb):
        return None, 0.0
    d2 = distance2(ka, ra, kb, rb)
    d = X.dec_sqrt(d2)
    return d, X.distance_bound(float(d), max(lmax(ka, ra), lmax(kb, rb)))


def rowwise(ka: int, rows_a, kb: int, rows_b, b_rows=None, valid_a=None, valid_b=None):
    """[(Decimal or None, bound)] of distance(a[i], b[b_rows[i]]); None for null, empty or out-of-range rows"""
    out = []
    for i, ra in enumerate(rows_a):
        j = i if b_rows is None else int(b_rows[i])
        if j >= len(rows_b) or (valid_a is not None and not valid_a[i]) or (valid_b is not None and not valid_b[j]):
            out.append((None, 0.0))
            continue
        out.append(distance(ka, ra, kb, rows_b[j]))
    return out


def check(got, exact, what=""):
    """GPU results against rowwise(): NaN where None; else zero exactly when the exact distance is zero, and within the a-priori
    bound (16 u (d + 2 lmax): tighter than 1e-9 relative wherever d is not tiny against the features' extent)"""
    assert len(got) == len(exact), what
    for i, (d, b) in enumerate(exact):
        if d is None:
            assert np.isnan(got[i]), (what, i, got[i])
            continue
        assert np.isfinite(got[i]), (what, i, got[i], d)
        assert (got[i] == 0.0) == (d == 0), (what, i, got[i], d)
        assert X.abs_err(got[i], d) <= b, (what, i, got[i], d, b)
