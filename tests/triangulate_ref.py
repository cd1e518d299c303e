"""Exact checker of gpk_triangulate (include/geopolars_hip.h, csrc/gpk_triangulate.h) and the plumbing of its tests.

A triangulation is not unique, so there is no golden answer: check_row decides, in exact integer arithmetic built straight from the
float coordinates (every finite float is an integer multiple of a power of two), whether a set of triangles satisfies the guarantee
(a) - (e) of the header for one row.  Directed-edge hashing keeps the conformity test linear in the triangle count; the vertex-on-edge
test is brute force behind a float filter whose misses are impossible (the filter's bound is far above the rounding of the float
determinant); rows of at most PAIRWISE_MAX triangles also get a brute-force test that no two triangle interiors meet.

Rows are what tests/validity_ref.py uses: a POLYGON row is a list of rings, a MULTIPOLYGON row a list of polygons."""
from __future__ import annotations

import math
import struct
from fractions import Fraction

import numpy as np

from geopolars_amd import _abi

PG, MPG = _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON
TRI_OK, TRI_EMPTY, TRI_FAILED = 0, 1, 2
# csrc/gpk_triangulate.h, restated
TRI_G_SMALL, TRI_G_LARGE, TRI_G_MEAN, TRI_SLICE_SMALL, TRI_SLICE_LARGE, TRI_LDS_NODES = 4, 16, 32.0, 32, 128, 5000
PAIRWISE_MAX = 200


class TriangulationError(AssertionError):
    pass


def members_of(kind, row):
    return [row] if kind == PG else list(row)


def row_rings(kind, row):
    """[(member number, ring number in the member, first coordinate index in the row, ring)] of every ring, empty ones included"""
    out, at = [], 0
    for m, poly in enumerate(members_of(kind, row)):
        for k, ring in enumerate(poly):
            out.append((m, k, at, ring))
            at += len(ring)
    return out


def share(kind, row) -> int:
    rr = row_rings(kind, row)
    return sum(len(r[3]) for r in rr) + 3 * len(rr)


def _ints(xy):
    """float coordinates as exact integers on one grid"""
    fr = [Fraction(float(v)) for p in xy for v in p]
    den = math.lcm(*[f.denominator for f in fr]) if fr else 1
    it = [int(f * den) for f in fr]
    return list(zip(it[0::2], it[1::2]))


def _orient(a, b, c):
    d = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    return (d > 0) - (d < 0)


def _area2(ring):
    return sum(p[0] * q[1] - p[1] * q[0] for p, q in zip(ring, ring[1:] + ring[:1]))


def _strictly_inside(p, a, b):
    """p in the open segment ab (integers)"""
    if p == a or p == b or _orient(a, b, p) != 0:
        return False
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def _near_segments(F, a_idx, b_idx, v_idx):
    """for every segment k (a_idx[k] -> b_idx[k], float coordinates F) the positions in v_idx of the vertices that may lie on it"""
    P, Q, V = F[a_idx], F[b_idx], F[v_idx]
    out = []
    for k in range(len(P)):
        d, w = Q[k] - P[k], V - P[k]
        cross = d[0] * w[:, 1] - d[1] * w[:, 0]
        bound = 1e-9 * (abs(d[0]) + abs(d[1])) * (np.abs(w[:, 0]) + np.abs(w[:, 1]) + abs(d[0]) + abs(d[1]))
        lo, hi = np.minimum(P[k], Q[k]), np.maximum(P[k], Q[k])
        m = (np.abs(cross) <= bound) & (V[:, 0] >= lo[0]) & (V[:, 0] <= hi[0]) & (V[:, 1] >= lo[1]) & (V[:, 1] <= hi[1])
        out.append(np.nonzero(m)[0])
    return out


def check_row(kind, row, tris, base=0, full=True):
    """raises TriangulationError unless `tris` ((T, 3) coordinate indices, the row's first coordinate being `base`) is a triangulation
    of the valid row under (a) - (e).  full=False: the linear-time part only ((a), (b), (d), the directed-edge part of (c))."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3) - base
    rings = [r for r in row_rings(kind, row)]
    flat = [tuple(map(float, p)) for r in rings for p in r[3]]
    n = len(flat)
    live = [r for r in rings if len(r[3]) and len(members_of(kind, row)[r[0]][0])]  # non-empty rings of non-empty members
    if not live:
        if len(tris):
            raise TriangulationError("triangles for a row without a non-empty member")
        return
    I = _ints(flat)
    F = np.array(flat, dtype=np.float64).reshape(-1, 2)
    ring_of = np.full(n, -1)
    closers = set()
    for k, (m, _, at, ring) in enumerate(rings):
        ring_of[at : at + len(ring)] = k
        if len(ring):
            closers.add(at + len(ring) - 1)
    # (a)
    if len(tris) and (tris.min() < 0 or tris.max() >= n):
        raise TriangulationError(f"(a) an index outside the row: {tris.min() + base} .. {tris.max() + base}, the row has {base} .. {base + n - 1}")
    bad = [int(i) + base for i in tris.ravel() if int(i) in closers]
    if bad:
        raise TriangulationError(f"(a) index of a closing coordinate: {bad[:4]}")
    # (b)
    for t in tris:
        if _orient(I[t[0]], I[t[1]], I[t[2]]) <= 0:
            raise TriangulationError(f"(b) triangle {t + base} is not strictly counter-clockwise")
    # (d) and the member of every triangle
    member_of_tri = [rings[ring_of[t[0]]][0] for t in tris]
    # (where members touch, a vertex of another member may stand in for the touch point: the counts are then compared row-wide)
    mixed = any(rings[ring_of[i]][0] != m for t, m in zip(tris, member_of_tri) for i in t)
    want = {}
    for m, k, at, ring in live:
        a2 = abs(_area2(I[at : at + len(ring) - 1]))
        want[m] = want.get(m, 0) + (a2 if k == 0 else -a2)
    got = {}
    for t, m in zip(tris, member_of_tri):
        a, b, c = I[t[0]], I[t[1]], I[t[2]]
        got[m] = got.get(m, 0) + (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    if sum(got.values()) != sum(want.values()):
        raise TriangulationError(f"(d) twice the area: triangles {sum(got.values())}, row {sum(want.values())} (on the row's integer grid)")
    # (c) directed edges by coordinate value
    edges = {}
    for t in tris:
        for u, v in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            key = (I[u], I[v])
            if key in edges:
                raise TriangulationError(f"(c) the directed edge {flat[u]} -> {flat[v]} occurs twice")
            edges[key] = (int(u), int(v))
    open_edges = [(k, uv) for k, uv in edges.items() if (k[1], k[0]) not in edges]
    seg_a, seg_b = [], []
    for m, k, at, ring in live:
        for j in range(len(ring) - 1):
            if I[at + j] != I[at + j + 1]:
                seg_a.append(at + j)
                seg_b.append(at + j + 1)
    whole = {(I[u], I[v]) for u, v in zip(seg_a, seg_b)}
    open_edges = [(k, uv) for k, uv in open_edges if k not in whole and (k[1], k[0]) not in whole]  # (a whole ring edge: nothing to search)
    seg_a, seg_b = np.array(seg_a), np.array(seg_b)
    if open_edges:
        ends = np.array([uv[0] for _, uv in open_edges] + [uv[1] for _, uv in open_edges])
        near = _near_segments(F, seg_a, seg_b, ends)
        on = [set() for _ in ends]  # ring segments that hold each end point (closed)
        for s, hits in enumerate(near):
            a, b = I[seg_a[s]], I[seg_b[s]]
            for h in hits:
                p = I[ends[h]]
                if p == a or p == b or _strictly_inside(p, a, b):
                    on[h].add(s)
        ne = len(open_edges)
        for e, (key, uv) in enumerate(open_edges):
            if not (on[e] & on[ne + e]):
                raise TriangulationError(f"(c) the edge {flat[uv[0]]} -> {flat[uv[1]]} has no reverse and lies on no ring edge")
    if not full:
        return
    # (c) no vertex of the row in the open interior of a triangle edge
    verts = np.array(sorted({at + j for m, k, at, ring in live for j in range(len(ring) - 1)}))
    ea = np.array([uv[0] for uv in edges.values()])
    eb = np.array([uv[1] for uv in edges.values()])
    if len(ea):
        for e, hits in enumerate(_near_segments(F, ea, eb, verts)):
            for h in hits:
                if _strictly_inside(I[verts[h]], I[ea[e]], I[eb[e]]):
                    raise TriangulationError(f"(c) vertex {flat[verts[h]]} lies inside the triangle edge {flat[ea[e]]} -> {flat[eb[e]]}: a T-junction")
    # (e) counts per member
    touch = _near_segments(F, seg_a, seg_b, verts)
    s_of = {}
    shared = False
    pos_ring = {}
    for v in verts:
        pos_ring.setdefault(I[v], set()).add(int(ring_of[v]))
    shared = any(len(s) > 1 for s in pos_ring.values())
    for s, hits in enumerate(touch):
        rs = ring_of[seg_a[s]]
        seen = set()
        for h in hits:
            v = verts[h]
            if ring_of[v] != rs and I[v] not in seen and _strictly_inside(I[v], I[seg_a[s]], I[seg_b[s]]):
                seen.add(I[v])  # (coincident vertices of several rings split the edge once)
                s_of[rings[rs][0]] = s_of.get(rings[rs][0], 0) + 1
                shared = True
    count = {}
    for m in member_of_tri:
        count[m] = count.get(m, 0) + 1
    bounds = {}
    for m in want:
        npos = 0
        holes = -1
        for mm, k, at, ring in live:
            if mm != m:
                continue
            holes += 1
            pts = [I[at + j] for j in range(len(ring) - 1)]
            pts = [p for j, p in enumerate(pts) if j == 0 or p != pts[j - 1]]
            while len(pts) > 1 and pts[-1] == pts[0]:
                pts.pop()
            npos += len(pts)
        bounds[m] = npos + s_of.get(m, 0) + 2 * holes - 2
    if mixed:
        bounds, count = {"row": sum(bounds.values())}, {"row": len(tris)}
    for m, bound in bounds.items():
        c = count.get(m, 0)
        if c > bound or (not shared and c != bound):
            raise TriangulationError(f"(e) member {m}: {c} triangles, {'at most' if shared else 'exactly'} {bound} expected")
    # interiors pairwise disjoint
    if len(tris) <= PAIRWISE_MAX:
        hit = first_overlap([(I[t[0]], I[t[1]], I[t[2]]) for t in tris])
        if hit is not None:
            raise TriangulationError(f"triangles {tris[hit[0]] + base} and {tris[hit[1]] + base} overlap")


def first_overlap(T):
    """the first pair (i, j) of counter-clockwise integer triangles whose interiors meet, or None: brute force over all pairs"""
    lo = [(min(p[0] for p in t), min(p[1] for p in t)) for t in T]
    hi = [(max(p[0] for p in t), max(p[1] for p in t)) for t in T]
    for i in range(len(T)):
        for j in range(i + 1, len(T)):
            if lo[i][0] >= hi[j][0] or lo[j][0] >= hi[i][0] or lo[i][1] >= hi[j][1] or lo[j][1] >= hi[i][1]:
                continue
            if not _separated(T[i], T[j]) and not _separated(T[j], T[i]):
                return i, j
    return None


def _separated(s, t):
    """an edge of the counter-clockwise triangle s has all of t on its right or on it"""
    for a, b in ((s[0], s[1]), (s[1], s[2]), (s[2], s[0])):
        if all(_orient(a, b, p) <= 0 for p in t):
            return True
    return False


def check_safe(kind, row, status, tris, base=0):
    """what holds for every row, valid or not: a known status, triangles only with GPK_TRI_OK, indices in the row, the count in the share"""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    n = sum(len(r[3]) for r in row_rings(kind, row))
    assert status in (TRI_OK, TRI_EMPTY, TRI_FAILED), status
    assert status == TRI_OK or len(tris) == 0, (status, len(tris))
    assert len(tris) <= share(kind, row), (len(tris), share(kind, row))
    if len(tris):
        assert tris.min() >= base and tris.max() < base + n, (tris.min(), tris.max(), base, n)


def has_member(kind, row, valid=True) -> bool:
    return bool(valid) and row is not None and any(len(p) and len(p[0]) for p in members_of(kind, row))


# ---- the host driver's records (tests/triangulate_host_driver.cpp) ------------------------------------------------------------------


def driver_records(kind, rows, valid=None) -> bytes:
    out = []
    for i, row in enumerate(rows):
        if row is None or (valid is not None and not valid[i]):
            out.append(struct.pack("<ii", int(kind == MPG), -1))
            continue
        ms = members_of(kind, row)
        out.append(struct.pack("<ii", int(kind == MPG), len(ms)))
        for p in ms:
            out.append(struct.pack("<i", len(p)))
            for ring in p:
                out.append(struct.pack("<i", len(ring)))
                out.append(np.asarray(ring, dtype=np.float64).reshape(-1, 2).tobytes())
    return b"".join(out)


def driver_answers(raw: bytes, n_rows: int):
    """[(status, (T, 3) row-local indices)]"""
    out, at = [], 0
    for _ in range(n_rows):
        status, nt = struct.unpack_from("<ii", raw, at)
        at += 8
        out.append((status, np.frombuffer(raw, dtype=np.uint32, count=3 * nt, offset=at).reshape(-1, 3).astype(np.int64)))
        at += 12 * nt
    assert at == len(raw)
    return out


def array_rows(arr):
    """(kind, rows) of a host POLYGON / MULTIPOLYGON GeoArrowArray"""
    xy, ro = arr.xy, arr.ring_offsets
    ring = lambda s: [tuple(map(float, p)) for p in xy[ro[s] : ro[s + 1]]]  # noqa: E731
    go = arr.geom_offsets
    if arr.geom_type == PG:
        return PG, [[ring(s) for s in range(go[i], go[i + 1])] for i in range(arr.n_geoms)]
    po = arr.part_offsets
    return MPG, [[[ring(s) for s in range(po[p], po[p + 1])] for p in range(go[i], go[i + 1])] for i in range(arr.n_geoms)]
