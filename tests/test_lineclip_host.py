"""The line clip, host side: the header's arithmetic (csrc/gpk_lineclip.h: the crossing point around a local origin, the order of events
with its exact tie rules, the run state machine) run on the CPU by a stand-alone program against the exact fixture — plain and under
AddressSanitizer + UBSan, at the lattice placement and at a georeferenced one — and the checks that need no device: the C ABI symbols,
the header's text, the refusals of the library that come before any device work, and the Python refusals that come before the library
is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import line_clip_pairs, spatial_join_clip
from tests import lineclip_ref as L
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "lineclip", fp_contract_off=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(L.GOLDEN)


CALL = np.dtype([("begin", np.int32), ("event", np.int32), ("x", np.float64), ("y", np.float64)])


def _off_segment(pt, u, v):
    e, w = v - u, pt - u
    s = min(1.0, max(0.0, float(w @ e) / float(e @ e)))
    return float(np.hypot(*(w - s * e)))


@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, golden, build, placement):
    """Every non-degenerate segment of every usable fixture pair, both modes: the driver gets the segment's touch points in reverse
    order with their exact types and must make the sink calls of the exact reference — the same structure, coordinates of the line and
    vertices of the polygon bit for bit, computed crossings within 1e-9 * d of the segment and of the ring edge.  The translation by
    (500000, 4649776) keeps the lattice exact: there the determinants of raw coordinates would lose the crossing parameter."""
    built, workdir = drivers
    offset = (0.0, 0.0) if placement == "lattice" else L.TRANSLATION
    worst, n_cross = 0.0, 0
    for kl, kp in L.FAMILIES:
        cl, cp = L.load(golden, kl, kp, offset)
        for mode in L.MODES:
            records, want = L.driver_case(kl, kp, mode, cl, cp)
            fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
            with open(fin, "wb") as f:
                f.write(records)
            r = subprocess.run([built[build], fin, fout], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            raw = open(fout, "rb").read()
            at = 0
            for calls, p, q, d, edges in want:
                n = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=at)[0])
                got = np.frombuffer(raw, dtype=CALL, count=n, offset=at + 4)
                at += 4 + n * CALL.itemsize
                assert [(int(g["begin"]), int(g["event"])) for g in got] == [(c[0], c[1]) for c in calls], (L.NAMES[kl], L.NAMES[kp], mode, p, q)
                for g, (_b, k, tag, x, y) in zip(got, calls):
                    if tag != L.TAG_X:
                        assert g["x"].tobytes() == np.float64(x).tobytes() and g["y"].tobytes() == np.float64(y).tobytes()
                    else:
                        a, b = edges[k]
                        pt = np.array([g["x"], g["y"]])
                        ratio = max(_off_segment(pt, p, q), _off_segment(pt, a, b)) / (L.REL_TOL * d)
                        worst, n_cross = max(worst, ratio), n_cross + 1
                        assert ratio <= 1.0, (ratio, pt, p, q, a, b)
            assert at == len(raw)
    assert n_cross > 1000
    print(f"worst (c) distance / (1e-9 d) over {n_cross} crossings, {placement}: {worst:.3e}")


def test_exact_tie_rules_of_the_event_order(drivers, tmp_path):
    """On a segment of length 3e12 the parameters of (3, 1), (6, 2) and of the crossing at (3, 1) are 1e-12 apart and a vertex has no
    parameter at all: the driver must order two vertices by coordinate and a vertex against a crossing by orientation, the vertex AT
    the crossing point first."""
    built, _ = drivers
    big = 3.0e12
    p, q = (0.0, 0.0), (big, big / 3.0)
    # the edge (2, 3) - (4, -1) crosses pq exactly at (3, 1); vertex events at (3, 1) and (6, 2), handed over last first
    rec = np.array([0, 0], dtype=np.int32).tobytes() + np.array([*p, *q, 0.0, 0.0], dtype=np.float64).tobytes() + np.array([3], dtype=np.int32).tobytes()
    for kind, typ, a, b in ((0, -1, (6.0, 2.0), (6.0, 2.0)), (0, 1, (3.0, 1.0), (3.0, 1.0)), (1, 1, (2.0, 3.0), (4.0, -1.0))):
        rec += np.array([kind, typ], dtype=np.int32).tobytes() + np.array([*a, *b], dtype=np.float64).tobytes()
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(rec)
    for exe in built.values():
        r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        raw = fout.read_bytes()
        got = np.frombuffer(raw, dtype=CALL, count=int(np.frombuffer(raw, dtype=np.int32, count=1)[0]), offset=4)
        # (3, 1) is AT the crossing point of this edge: the vertex comes first, then the crossing, then (6, 2) — depth 1, 2, 1: one
        # part from (3, 1), not closed by (6, 2), closed by q
        assert [(int(g["begin"]), int(g["event"])) for g in got] == [(1, 1), (0, -1)], got
        assert (got[0]["x"], got[0]["y"]) == (3.0, 1.0) and (got[1]["x"], got[1]["y"]) == q


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_exported_symbols_name_the_clip_call():
    assert "gpk_line_clip" in _abi.EXPORTED_SYMBOLS
    args = _abi._PROTOS["gpk_line_clip"][1]
    assert len(args) == 12 and args[4] is C.c_int64
    assert (_abi.CLIP_INSIDE, _abi.CLIP_OUTSIDE, _abi.CLIP_DROP_EMPTY) == (0, 1, 1)


def test_built_library_exports_the_clip_call():
    assert "gpk_line_clip" in exported_symbols()


def test_header_states_the_call_the_rows_and_the_contract():
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert ("int32_t gpk_line_clip(const gpk_geoarray* lines, const gpk_geoarray* polys, const uint32_t* line_rows, const uint32_t* poly_rows, "
            "int64_t n_rows, int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, void* stream, "
            "gpk_geoarray** out);") in flat
    for line in ("#define GPK_CLIP_INSIDE 0", "#define GPK_CLIP_OUTSIDE 1", "#define GPK_CLIP_DROP_EMPTY 1", "swap the arguments",
                 "a valid row with zero parts", "index past the end of its column", "1e-9 * d", "1e-6 * |segment|",
                 "a stretch the line covers twice is emitted twice", "correct and slow"):
        assert line in flat, line
    rule = " ".join(open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_lineclip.h")).read().split())
    for line in ("A segment pq with p == q is skipped", "depth", "they can never invert the", "always terminates",
                 "v lies before the crossing of ab iff orient(a, b, v) has the sign of orient(a, b, p)"):
        assert line in rule, line


@pytest.mark.parametrize("mode,flags,src,n", [(2, 0, None, 0), (-1, 0, None, 0), (0, 2, None, 0), (1, 3, None, 0), (0, 0, 64, 0), (0, 1, None, -1)])
def test_bad_plain_arguments_are_refused_by_the_library_before_any_device_work(mode, flags, src, n):
    """an unknown mode, unknown flag bits, out_src without DROP_EMPTY, a negative count: refused with not even a handle handed over"""
    out = C.c_void_p(7)
    rc = _abi.lib().gpk_line_clip(None, None, None, None, n, _abi.MEM_HOST, mode, flags, src, _abi.MEM_HOST, None, C.byref(out))
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT and "line_clip" in _abi.last_error()


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    return pts, lines, GeoSeries(GeoArrowArray.from_polygons([sq, sq, sq])), GeoSeries(GeoArrowArray.from_polygons([sq, sq]))


def test_family_and_shape_errors_come_before_the_device(no_device):
    pts, lines, polys, two = _series()
    for call in (lambda: polys.intersection(lines), lambda: polys.intersection(polys), lambda: lines.intersection(lines),
                 lambda: pts.intersection(polys), lambda: lines.difference(pts), lambda: polys.difference(polys),
                 lambda: line_clip_pairs(polys, lines, [0], [0]), lambda: line_clip_pairs(pts, polys, [0], [0]),
                 lambda: spatial_join_clip(polys, polys), lambda: spatial_join_clip(lines, pts)):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    with pytest.raises(_abi.MismatchedGeometry, match="swap"):
        polys.intersection(lines)
    with pytest.raises(_abi.MismatchedGeometry, match="intersection_area / intersection_length"):
        polys.difference(polys)
    for call in (
        lambda: lines.intersection(two),  # 3 rows against 2
        lambda: lines.intersection(two, other_rows=[0, 1]),  # one entry per row of self
        lambda: lines.difference(two, other_rows=["a", "b", "c"]),
        lambda: line_clip_pairs(lines, polys, [0, 1], [0]),
        lambda: line_clip_pairs(lines, polys, [0], [0], how="union"),
        lambda: line_clip_pairs(lines, polys, ["a"], ["b"]),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None and polys._dev is None and two._dev is None


def test_no_pair_needs_no_device(no_device):
    _pts, lines, polys, _two = _series()
    out, src = line_clip_pairs(lines, polys, [], [], drop_empty=True)
    assert len(out) == 0 and len(src) == 0 and out.array.geom_type == _abi.GEOM_MULTILINESTRING
