"""GPU: gpk_simplify (rdp_kernel<8|64>, rdp_compact_kernel<8|64>) against the exact reference of tests/simplify_ref.py on the
sequences that reference is entitled to judge (share asserted first) AND bit for bit against the CPU oracle on all of them: exact
ties across the lanes of a group, the closed threshold, the ring rule under divergence, shapes against each instance's grain, deep
explicit stacks with a wrapping grid, randomized lattice columns of all four families, the C ABI's variants, magnitudes.  Every case
runs in both instances: the column is padded until `simplify_group_size` gives 8 and then 64."""
import ctypes as C
import math

import numpy as np
import pytest

from geopolars_amd import _abi, synth
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from tests import exact_ref as X
from tests import simplify_ref as R

pytestmark = pytest.mark.gpu

LS, MLS, PG, MPG = R.LS, R.MLS, R.PG, R.MPG


def check(oracle, a: GeoArrowArray, eps, G=None, cap=R.CAP, what=""):
    """GeoSeries.simplify on the GPU: exact reference on the settled sequences (cap first), the oracle on all, nesting untouched"""
    if G is not None:
        assert R.group_size_of(a) == G, (what, "the column does not reach the instance it is meant for")
    got = GeoSeries(a).simplify(eps).array
    xy, off = got.xy, R.inner_offsets(got)
    share, res = R.compare_exact(a, eps, xy, off, cap=cap, what=(what, G))
    oxy, ooff = oracle.simplify(a, eps)
    assert np.array_equal(off, ooff) and np.array_equal(xy, oxy), (what, G, eps)
    assert got.geom_type == a.geom_type and got.n_geoms == a.n_geoms
    if a.ring_offsets is not None:
        assert np.array_equal(got.geom_offsets, a.geom_offsets)
        assert (got.part_offsets is None) == (a.part_offsets is None) and (a.part_offsets is None or np.array_equal(got.part_offsets, a.part_offsets))
    assert np.array_equal(got.is_valid(), a.is_valid())
    return share, res, got


def both_instances(oracle, kind, seqs, eps_values, cap=R.CAP, what="", null_every=0):
    out = []
    for G in (8, 64):
        a = R.as_column(kind, R.force_instance(seqs, G, ring=kind in (PG, MPG)), null_every=null_every)
        for eps in eps_values:
            out.append(check(oracle, a, eps, G=G, cap=cap, what=what))
    return out


# ---- exact ties ------------------------------------------------------------------------------------------------------------------
H = 0.25
BELOW = math.nextafter(H, 0.0)


def _tie_sweep(G):
    """(sequence, tied indices) for every length and placement of the sweep, for a G-wide group"""
    cases = []
    for n in (3, 4, G, G + 1, G + 2, 2 * G - 1, 2 * G, 2 * G + 1, 5 * G + 3):
        if n == 3:
            cases.append((R.tie_line(3, [1]), [1]))
        for k1, k2 in R.tie_pairs(n, G).values():
            for signs in ((1, 1), (1, -1), (-1, 1)):
                cases.append((R.tie_line(n, [k1, k2], signs=signs), [k1, k2]))
            if k2 - k1 >= 2:
                mid = (k1 + k2) // 2
                cases.append((R.tie_line(n, [k1, mid, k2], low=0.125), [k1, mid, k2]))
        if n > 8:  # ties in every lane and every pass: all interior points at +-h
            cases.append((R.tie_line(n, list(range(1, n - 1)), signs=[1 if k % 3 else -1 for k in range(1, n - 1)]), list(range(1, n - 1))))
    return cases


@pytest.mark.parametrize("G", [8, 64])
@pytest.mark.parametrize("kind", [LS, MLS])
def test_exact_ties_take_the_last_index_in_every_instance(gpk, oracle, kind, G):
    cases = _tie_sweep(G)
    seqs = [s for s, _ in cases] + [R.collinear_line(n) for n in range(3, G)]  # all distances 0.0: the idle lanes' (0.0, 0) take part
    for (share, res, got) in both_instances(oracle, kind, seqs, (BELOW, H, 0.125, 2.0**-30), cap=0.0, what=f"tie sweep {G}"):
        assert share == 0.0
    # what the sweep is built to give, said outright: just under the tied height the split happens at the LAST tied point, the rest
    # (nearer than h to both new chords) is culled; at the tied height nothing splits
    for Gi in (8, 64):
        a = R.as_column(kind, R.force_instance(seqs, Gi))
        lo, at = GeoSeries(a).simplify(BELOW).array, GeoSeries(a).simplify(H).array
        lo_off, at_off = R.inner_offsets(lo), R.inner_offsets(at)
        for i, (s, ties) in enumerate(cases):
            assert at.xy[at_off[i] : at_off[i + 1]].tolist() == [list(s[0]), list(s[-1])], (Gi, i)
            if len(ties) == 2 and s[ties[0]][1] == s[ties[1]][1]:  # (tied on the same side of the chord)
                assert lo.xy[lo_off[i] : lo_off[i + 1]].tolist() == [list(s[0]), list(s[ties[-1]]), list(s[-1])], (Gi, i, ties)
        for i in range(len(cases), len(cases) + G - 3):
            assert at_off[i + 1] - at_off[i] == 2 and lo_off[i + 1] - lo_off[i] == 2


@pytest.mark.parametrize("kind", [LS, MLS, PG, MPG])
def test_tie_families(gpk, oracle, kind):
    fam = R.tie_family_rings() if kind in (PG, MPG) else R.tie_family_lines()
    n_ties = 0
    for eps in sorted({e for _, _, es in fam for e in es}):
        seqs = [s for _, s, es in fam if eps in es]
        for share, res, _ in both_instances(oracle, kind, seqs * 3, (eps,), cap=0.0, what=f"family {kind}"):
            n_ties += sum(r.ties for r in res)
    assert n_ties > 100


def test_threshold_is_closed_and_unordered_eps_culls(gpk, oracle):
    line, ring = R.tie_line(40, [3, 18, 35]), R.circle_ring(3)
    for G in (8, 64):
        a = R.as_column(LS, R.force_instance([line, R.comb(20), R.staircase(8)], G))
        p = R.as_column(PG, R.force_instance([ring, R.sliver_ring(5, 7), R.rectangle_with_midpoints(m=7)], G, ring=True))
        n_line, n_ring = len(R.sequences(a)), len(R.sequences(p))
        for eps in (H, BELOW, 65.0, math.nextafter(65.0, 0.0)):
            check(oracle, a, eps, G=G, cap=0.0)
            check(oracle, p, eps, G=G, cap=0.0)
        assert R.inner_offsets(GeoSeries(a).simplify(H).array)[1] == 2 and R.inner_offsets(GeoSeries(a).simplify(BELOW).array)[1] == 3
        assert R.inner_offsets(GeoSeries(p).simplify(65.0).array)[1] == len(ring)  # d == eps: one range, refused by the floor of 4
        assert R.inner_offsets(GeoSeries(p).simplify(math.nextafter(65.0, 0.0)).array)[1] == 14
        for eps in (math.inf, math.nan):  # nothing is `> eps`: lines cull to 2, a ring's one range is refused
            _, _, got = check(oracle, a, eps, G=G, cap=0.0)
            assert np.array_equal(np.diff(R.inner_offsets(got)), np.minimum(np.diff(R.inner_offsets(a)), 2))
            _, _, got = check(oracle, p, eps, G=G, cap=0.0)
            assert np.array_equal(got.xy, p.xy)
        for eps in (0.0, -0.0, -1.0, -math.inf):
            _, _, got = check(oracle, a, eps, G=G, cap=0.0)
            assert np.array_equal(got.xy, a.xy)
        assert n_line >= 3 and n_ring >= 3


# ---- the ring rule -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [PG, MPG])
def test_ring_rule_with_diverging_groups(gpk, oracle, kind):
    rings = [r for _, ring in R.order_rings() for r in (ring, ring[::-1])]
    rng = np.random.default_rng(3)
    seqs = [rings[i] for i in rng.integers(0, len(rings), 40 * len(rings))]  # neighbours in a wave walk different trees
    both = 0
    for share, res, got in both_instances(oracle, kind, seqs, (R.ORDER_EPS, 1e300), cap=0.0, what="ring rule", null_every=5):
        assert np.all(np.diff(R.inner_offsets(got))[: len(seqs)] >= 4)
        both += sum(r.refused_ranges > 0 and r.culled_ranges > 0 for r in res)
    assert both > 100  # rings in which one range culled and a later one was refused


# ---- shapes against the instance's grain -------------------------------------------------------------------------------------


def test_a_long_ring_in_the_narrow_instance(gpk, oracle):
    rng = np.random.default_rng(9)
    w = np.cumsum(rng.integers(-50, 51, (19_999, 2)), axis=0).astype(np.float64)
    ring = np.concatenate([w, w[:1]])
    small = R.lattice_sequences(60, 4, ring=True, hi=30)
    seqs = [ring] + small + [[]] * 400  # mean (20 000 + ~1 000) / 461 <= 48
    a = R.as_column(PG, seqs, null_every=4)
    assert R.group_size_of(a) == 8
    for eps in (7.0, 2000.0):
        share, res, got = check(oracle, a, eps, G=8, what="long ring")
        assert res[0].settled and res[0].nodes > (1000 if eps == 7.0 else 10)
        R.check_sequence_properties(ring, got.xy[: R.inner_offsets(got)[1]], eps, 4)


@pytest.mark.parametrize("kind", [LS, MLS, PG, MPG])
def test_short_sequences_in_the_wide_instance(gpk, oracle, kind):
    ring = kind in (PG, MPG)
    longs = R.lattice_sequences(12, 6, ring=ring, lo=150, hi=400)
    shorts = [[], [(1.0, 2.0)], [(1.0, 2.0), (3.0, 4.0)], [(0.0, 0.0), (4.0, 1.0), (0.0, 0.0)] if ring else [(0.0, 0.0), (4.0, 1.0), (8.0, 0.0)], []]
    seqs = []
    for q, s in enumerate(longs):
        seqs += [s, shorts[q % len(shorts)]]
    seqs = shorts + seqs + shorts
    a = R.as_column(kind, seqs, null_every=3)
    assert R.group_size_of(a) == 64 and not a.is_valid().all()
    for eps in (2.5, 7.0, 300.0):
        _, _, got = check(oracle, a, eps, G=64, what="short among long")
        for i, s in enumerate(seqs):
            if len(s) < 3:
                assert np.diff(R.inner_offsets(got))[i] == len(s)


# ---- deep stacks, wrapping grids ------------------------------------------------------------------------------------------------


def _tiled_column(distinct, n_seq, inserts):
    """n_seq sequences cycling through `distinct`, with `inserts` {position: sequence} put in — assembled in numpy"""
    order = [np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in distinct]
    picks = [inserts[i] if i in inserts else order[i % len(order)] for i in range(n_seq)]
    picks = [np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in picks]
    off = np.concatenate([[0], np.cumsum([len(s) for s in picks])]).astype(np.int32)
    return GeoArrowArray(LS, np.concatenate(picks), geom_offsets=off)


@pytest.mark.parametrize("G", [8, 64])
def test_deep_stacks_and_a_wrapping_grid(gpk, oracle, G):
    _, cus = gpk.device_info()
    groups = cus * 32 * (256 // G)  # group_grid caps the blocks at cu_count * 32: sequences beyond this many are met on a later trip
    n_seq = groups + groups // 8 + 5
    spiral = R.square_spiral(3000)
    if G == 8:
        distinct = [R.tie_line(n, [1, n - 2]) for n in (3, 4, 5, 7, 9)] + [R.collinear_line(4), [], [(1.0, 1.0)]]
    else:
        distinct = [R.tie_line(n, [2, n // 2, n - 3], low=0.125) for n in (60, 64, 65, 70)] + [R.comb(20), R.staircase(30)]
    a = _tiled_column(distinct, n_seq, {0: spiral, 7: spiral[::-1], groups - 1: spiral, groups + 3: spiral, n_seq - 1: spiral})
    assert R.group_size_of(a) == G
    for eps, depth in ((BELOW, 2990), (375.0, 1500), (1e9, 0)):  # keep-all, part, cull-all
        share, res, got = check(oracle, a, eps, G=G, cap=0.0, what="deep")
        assert res[0].depth >= depth and res[-1].depth >= depth
        k = int(res[0].keep.sum())
        assert np.diff(R.inner_offsets(got))[[0, groups - 1, groups + 3, n_seq - 1]].tolist() == [k] * 4


# ---- randomized columns --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [LS, MLS, PG, MPG])
def test_random_lattice_columns(gpk, oracle, kind):
    seqs = R.lattice_sequences(120, 20 + kind, ring=kind in (PG, MPG))
    shares = [s for s, _, _ in both_instances(oracle, kind, seqs, R.LATTICE_EPS, what=f"lattice {kind}", null_every=7)]
    print(f"lattice kind {kind}: largest unsettled share {max(shares)}")


@pytest.mark.parametrize("eps", [0.05, 0.8, 4.0, 50.0])
def test_float_columns_against_the_rationals(gpk, oracle, eps):
    """the generators of test_simplify_parity, at a size the rationals can walk"""
    for a in (synth.random_linestrings(300), synth.clustered_polygons(400, seed=8), synth.powerlaw_multipolygons(200)):
        share, _, _ = check(oracle, a, eps, what="float columns")
        assert share <= 0.01


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------


def _abi_simplify(handle, eps, n_coords, n_seq, fill=True, stream=None):
    xy = np.full((max(n_coords, 1), 2), -7.0)
    off = np.full(n_seq + 1, -7, dtype=np.int32)
    n_out = C.c_int64(-1)
    rc = _abi.lib().gpk_simplify(handle, float(eps), xy.ctypes.data if fill else None, off.ctypes.data, C.byref(n_out), _abi.MEM_HOST, stream)
    return rc, xy, off, int(n_out.value)


@pytest.mark.parametrize("G", [8, 64])
def test_abi_size_query_device_outputs_streams(gpk, oracle, G):
    import torch

    seqs = R.force_instance(R.lattice_sequences(150, 31, ring=True) + [R.circle_ring(3), [], [(0.0, 0.0)]], G, ring=True)
    a = R.as_column(MPG, seqs, null_every=4)
    assert R.group_size_of(a) == G
    s = GeoSeries(a)
    h, nc, ns = s.device().handle, a.n_coords, len(seqs)
    oxy, ooff = oracle.simplify(a, 7.0)
    rc, xy, off, n_out = _abi_simplify(h, 7.0, nc, ns)
    assert rc == 0 and n_out == ooff[-1] and np.array_equal(off, ooff) and np.array_equal(xy[:n_out], oxy) and np.all(xy[n_out:] == -7.0)
    rc, xy0, off0, n0 = _abi_simplify(h, 7.0, nc, ns, fill=False)  # the size query: offsets and the total, no coordinates
    assert rc == 0 and n0 == n_out and np.array_equal(off0, off) and np.all(xy0 == -7.0)
    rc, xy2, off2, n2 = _abi_simplify(h, 7.0, nc, ns)  # the same bytes again (the workspace is reused)
    assert rc == 0 and n2 == n_out and xy2.tobytes() == xy.tobytes() and off2.tobytes() == off.tobytes()
    dev = "cuda:0"
    side = torch.cuda.Stream(device=dev)
    for st in (torch.cuda.current_stream(), side):
        dxy = torch.full((nc, 2), -7.0, dtype=torch.float64, device=dev)
        doff = torch.full((ns + 1,), -7, dtype=torch.int32, device=dev)
        st.wait_stream(torch.cuda.current_stream())
        n_dev = C.c_int64(-1)
        _abi.check(_abi.lib().gpk_simplify(h, 7.0, C.c_void_p(dxy.data_ptr()), C.c_void_p(doff.data_ptr()), C.byref(n_dev), _abi.MEM_DEVICE, C.c_void_p(st.cuda_stream)))
        st.synchronize()
        assert n_dev.value == n_out and doff.cpu().numpy().tobytes() == off.tobytes() and dxy.cpu().numpy().tobytes() == xy[:nc].tobytes()
        n_dev = C.c_int64(-1)
        doff.fill_(-7)
        st.wait_stream(torch.cuda.current_stream())
        _abi.check(_abi.lib().gpk_simplify(h, 7.0, None, C.c_void_p(doff.data_ptr()), C.byref(n_dev), _abi.MEM_DEVICE, C.c_void_p(st.cuda_stream)))
        st.synchronize()
        assert n_dev.value == n_out and doff.cpu().numpy().tobytes() == off.tobytes()
    rc, xy3, off3, n3 = _abi_simplify(h, 7.0, nc, ns, stream=C.c_void_p(side.cuda_stream))  # host outputs through a stream of the caller's
    assert rc == 0 and xy3.tobytes() == xy.tobytes() and off3.tobytes() == off.tobytes()


def test_abi_zero_rows_and_refusals(gpk):
    for kind in (LS, MLS, PG, MPG):
        empty = GeoSeries(X.column(kind, []))
        rc, xy, off, n_out = _abi_simplify(empty.device().handle, 1.0, 0, 0)
        assert rc == 0 and n_out == 0 and off.tolist() == [0]
        assert len(empty.simplify(1.0)) == 0
        hollow = GeoSeries(X.column(kind, [[], []]))  # rows, no sequence below them (a linestring column: two empty sequences)
        out = hollow.simplify(1.0).array
        assert out.n_coords == 0 and len(out) == 2
    pts, mpts = GeoSeries(synth.uniform_points(5)), GeoSeries(X.column(_abi.GEOM_MULTIPOINT, [[(0.0, 0.0), (1.0, 1.0), (2.0, 0.0)], []]))
    for s, n_seq in ((pts, 5), (mpts, 2)):
        rc, _, _, _ = _abi_simplify(s.device().handle, 1.0, 5, n_seq)
        assert rc == _abi.GPK_ERR_MISMATCHED_GEOMETRY
        out = s.simplify(1.0).array  # the series passes them through
        assert np.array_equal(out.xy, s.array.xy) and out.geom_type == s.array.geom_type
    ok = GeoSeries(X.column(LS, [R.tie_line(5, [2])]))
    n_out = C.c_int64(0)
    off = np.zeros(2, dtype=np.int32)
    assert _abi.lib().gpk_simplify(ok.device().handle, 1.0, None, None, C.byref(n_out), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert _abi.lib().gpk_simplify(ok.device().handle, 1.0, None, off.ctypes.data, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT


# ---- magnitudes ------------------------------------------------------------------------------------------------------------------


def _moved(a: GeoArrowArray, scale=1.0, t=(0.0, 0.0)) -> GeoArrowArray:
    xy = a.xy * scale + np.asarray(t)
    assert np.array_equal((xy - np.asarray(t)) / scale, a.xy)  # the move itself is exact
    return GeoArrowArray(a.geom_type, xy, a.geom_offsets, a.part_offsets, a.ring_offsets, a.validity, n_geoms=a.n_geoms)


@pytest.mark.parametrize("kind", [LS, PG])
def test_scaled_and_translated_columns(gpk, oracle, kind):
    ring = kind == PG
    fam = R.tie_family_rings() if ring else R.tie_family_lines()
    eps_of = {"ties": (H, BELOW, 65.0, math.nextafter(65.0, 0.0), 1.0), "lattice": (2.5, 7.0)}
    cols = {"ties": [s for _, s, _ in fam], "lattice": R.lattice_sequences(60, 77, ring=ring)}
    for name, seqs in cols.items():
        for G in (8, 64):
            a = R.as_column(kind, R.force_instance(seqs, G, ring=ring))
            for eps in eps_of[name]:
                base = GeoSeries(a).simplify(eps).array
                for k in (30, -60):  # a power of two moves no mantissa: the same indices are kept
                    f = 2.0**k
                    _, _, got = check(oracle, _moved(a, scale=f), eps * f, G=G, cap=0.0 if name == "ties" else R.CAP, what=f"scaled {k}")
                    assert np.array_equal(R.inner_offsets(got), R.inner_offsets(base)) and np.array_equal(got.xy, base.xy * f)
                for t in X.LATTICE_OFFSETS:  # the exact reference of the translated input (the f64 decisions there are its own)
                    check(oracle, _moved(a, t=t), eps, G=G, what=f"translated {t}")
