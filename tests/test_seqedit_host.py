"""segmentize, remove_repeated_points, reverse and orient_polygons, host side: the host-callable routines of csrc/gpk_seqedit.h (piece
count, interpolation, keep test, the sources of a strip, the reversed source, the argmin with several group sizes, the neighbours of
the turn) run on the CPU by a stand-alone program — plain and under AddressSanitizer + UBSan — against tests/seqedit_ref.py, bit for
bit; and the checks that need no device: the C ABI symbols, the header's text, the refusals of the library that come before any device
work, and the Python refusals that come before the library is opened."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from tests import geotake_cases as K
from tests import seqedit_ref as R
from tests.second_pass import same_bits
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("gpk_segmentize", "gpk_remove_repeated_points", "gpk_reverse", "gpk_orient_polygons")
SEGMENTIZE, DEDUP, REVERSE, ORIENT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "seqedit", fp_contract_off=False)


def _levels(a: GeoArrowArray):
    return [o for o in (a.geom_offsets, a.part_offsets, a.ring_offsets) if o is not None]


def _run_driver(exe, workdir, host: GeoArrowArray, op, m=0.0, per_row=None, exterior_cw=False, group=8):
    """-> (innermost offsets, xy, reversed flags or None), or None when the driver reports an i32 overflow"""
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    levels = _levels(host)
    with open(fin, "wb") as f:
        f.write(struct.pack("<iiqdiiii", op, len(levels), len(host), float(m), int(per_row is not None), int(exterior_cw), group, 0))
        for o in levels:
            f.write(struct.pack("<q", len(o)) + o.astype("<i4").tobytes())
        f.write(struct.pack("<q", host.n_coords) + host.xy.tobytes())
        if per_row is not None:
            f.write(np.asarray(per_row, "<f8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(fout, "rb").read()
    (status,) = struct.unpack_from("<i", raw, 0)
    if status != 0:
        assert len(raw) == 4
        return None
    at = 4
    (n,) = struct.unpack_from("<q", raw, at)
    off = np.frombuffer(raw, "<i4", n, at + 8)
    at += 8 + 4 * n
    (n,) = struct.unpack_from("<q", raw, at)
    xy = np.frombuffer(raw, "<f8", 2 * n, at + 8).reshape(-1, 2)
    at += 8 + 16 * n
    rev = None
    if op == ORIENT:
        (n,) = struct.unpack_from("<q", raw, at)
        rev = np.frombuffer(raw, np.uint8, n, at + 8).astype(bool)
        at += 8 + n
    assert at == len(raw)
    return off, xy, rev


def _same(got, want: GeoArrowArray, what):
    off, xy, _ = got
    assert np.array_equal(off, _levels(want)[-1]), what
    assert same_bits(xy, want.xy), what


COLUMNS = {k: v for k, v in K.columns().items() if v.geom_type in R.EDITED}
COLUMNS.update({k: v for k, v in K.edge_columns().items() if v.geom_type in R.EDITED})
COLUMNS.update(R.case_columns())
BUILDS = ["plain", "sanitized"]


@pytest.mark.parametrize("build", BUILDS)
def test_segmentize_driver_matches_the_reference(drivers, build):
    """every column with a bound that splits many segments, the hand-built shapes with their own bounds, per-row bounds with NaN / 0 /
    negative entries, and the overflow of i32 offsets"""
    built, workdir = drivers
    for name, host in COLUMNS.items():
        _same(_run_driver(built[build], workdir, host, SEGMENTIZE, m=7.5), R.segmentize(host, 7.5), name)
    for name, (host, m) in R.segmentize_cases().items():
        _same(_run_driver(built[build], workdir, host, SEGMENTIZE, m=m), R.segmentize(host, m), name)
    for name in ("linestring", "multipolygon+nulls", "polygon empty run", "segmentize: zero-length segment"):
        host = COLUMNS[name]
        per_row = np.random.default_rng(len(name)).uniform(1.0, 30.0, len(host))
        per_row[::5], per_row[1::7], per_row[2::9] = np.nan, 0.0, -3.0
        _same(_run_driver(built[build], workdir, host, SEGMENTIZE, per_row=per_row), R.segmentize(host, per_row), (name, "per row"))
    assert _run_driver(built[build], workdir, R.linestrings([[(0, 0), (1e10, 0)]]), SEGMENTIZE, m=1.0) is None
    with pytest.raises(OverflowError):
        R.segmentize(R.linestrings([[(0, 0), (1e10, 0)]]), 1.0)


@pytest.mark.parametrize("build", BUILDS)
def test_dedup_and_reverse_drivers_match_the_reference(drivers, build):
    built, workdir = drivers
    for name, host in COLUMNS.items():
        _same(_run_driver(built[build], workdir, host, DEDUP), R.remove_repeated_points(host), (name, "dedup"))
        _same(_run_driver(built[build], workdir, host, REVERSE), R.reverse(host), (name, "reverse"))


@pytest.mark.parametrize("build", BUILDS)
def test_orient_driver_matches_the_reference_with_every_group_size(drivers, build):
    """the argmin reduced by 1, 8, 64 and 256 lanes a ring gives the same decisions and the same column"""
    built, workdir = drivers
    for name, host in COLUMNS.items():
        if host.geom_type not in (_abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON):
            continue
        for cw in (False, True):
            want_rev, want = R.orient_decisions(host, cw), R.orient_polygons(host, cw)
            for group in (1, 8, 64, 256):
                got = _run_driver(built[build], workdir, host, ORIENT, exterior_cw=cw, group=group)
                assert np.array_equal(got[2], want_rev), (name, cw, group)
                _same(got, want, (name, cw, group))


def test_the_hand_built_shapes_say_what_they_claim():
    text = open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_seqedit.h")).read()
    assert "constexpr int STRIP = gt::STRIP;" in text and "constexpr int SOURCES = STRIP + 1;" in text and R.STRIP == K.STRIP == 1024
    seg = R.segmentize_cases()
    for name, total in (("1025 outputs of one segment", 1025), ("1024 outputs of one segment", 1024), ("1023 outputs of one segment", 1023),
                        ("1025 unsplit coordinates", 1025), ("5000 pieces between unsplit neighbours", 5003)):
        assert R.segmentize(*seg[name]).n_coords == total, name
    boundary = R.segmentize(*seg["sequence boundary at the strip boundary"])
    assert boundary.ring_offsets[1] == R.STRIP and boundary.n_coords > R.STRIP + 10
    host, m = seg["m larger than every segment"]
    assert same_bits(R.segmentize(host, m).xy, host.xy)
    assert 0.3 / 0.1 == 2.9999999999999996 and list(np.diff(R.segmentize(*seg["0.3 / 0.1"]).geom_offsets)) == [4, 4]
    nan = R.segmentize(*seg["NaN and inf"])
    assert nan.n_coords == 6 + 4  # only (9, 9) -> (12, 13), of length 5, is split
    geo = R.segmentize(*seg["georeferenced"])
    assert geo.n_coords > 150 and same_bits(geo.xy[[0, -1]], seg["georeferenced"][0].xy[[0, -1]])
    # the sliver: the f64 shoelace sum disagrees with the exact sign, which decides
    ring, exact = R.sliver()
    f = R.shoelace(ring)
    assert exact != 0 and (f > 0) - (f < 0) != exact
    dd = R.dedup_cases()
    assert R.remove_repeated_points(dd["a run across 1024"]).n_coords == 1100 - 19
    assert list(np.diff(R.remove_repeated_points(dd["repeats across a sequence boundary"]).ring_offsets)) == [4, 4]
    assert R.remove_repeated_points(dd["-0.0 after 0.0"]).n_coords == 2 and R.remove_repeated_points(dd["NaN after NaN"]).n_coords == 5
    assert list(np.diff(R.remove_repeated_points(dd["a collapsed ring"]).ring_offsets)) == [1, 4]
    rv = R.reverse_cases()
    assert np.count_nonzero(np.diff(rv["5000 empty sequences"].geom_offsets) == 0) > K.WINDOW + 2
    oc = R.orient_cases()
    assert list(R.orient_decisions(oc["squares and holes both ways"])) == [False, True, False, True, False, False, True, True, True, False]
    assert list(R.orient_decisions(oc["squares and holes both ways"], True)) == [True, False, True, False, True, True, False, False, False, True]
    assert list(R.orient_decisions(oc["smallest repeated"])) == [False, True, False, True]
    for name in ("spike", "NaN ring", "inf closing"):
        assert not R.orient_decisions(oc[name]).any() and not R.orient_decisions(oc[name], True).any(), name
    assert list(R.orient_decisions(oc["3-coordinate ring"])) == [False, True]
    assert list(R.orient_decisions(oc["5000-coordinate rings"])) == [False, False, False, False, True, False]
    assert list(R.orient_decisions(oc["rings of 256 and 257 coordinates"])) == [True, True, False, False]
    assert "constexpr int SHORT_RING = 256;" in open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_seqedit.hip")).read()
    assert list(R.orient_decisions(oc["sliver"])) == [exact < 0, exact > 0]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_exported_symbols_name_the_four_calls():
    for name in NAMES:
        assert name in _abi.EXPORTED_SYMBOLS
    assert len(_abi._PROTOS["gpk_segmentize"][1]) == 6 and _abi._PROTOS["gpk_segmentize"][1][1] is C.c_double
    assert len(_abi._PROTOS["gpk_remove_repeated_points"][1]) == 4 and len(_abi._PROTOS["gpk_reverse"][1]) == 3
    assert len(_abi._PROTOS["gpk_orient_polygons"][1]) == 4


def test_built_library_exports_the_four_calls():
    from geopolars_amd import build

    names = exported_symbols()
    assert set(NAMES) <= names
    assert "gpk_seqedit.hip" in build.SOURCES


def test_header_states_the_four_calls_and_the_contract():
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().replace(" * ", " ").split())
    for proto in ("int32_t gpk_segmentize(const gpk_geoarray* a, double max_segment_length, const double* per_row, int32_t per_row_space, void* stream, gpk_geoarray** out);",
                  "int32_t gpk_remove_repeated_points(const gpk_geoarray* a, double tolerance, void* stream, gpk_geoarray** out);",
                  "int32_t gpk_reverse(const gpk_geoarray* a, void* stream, gpk_geoarray** out);",
                  "int32_t gpk_orient_polygons(const gpk_geoarray* a, int32_t exterior_cw, void* stream, gpk_geoarray** out);"):
        assert proto in flat, proto
    for line in ("Every geometry type is accepted", "a may be freed first", "copied unchanged", "exactly when a has one", "keep their (empty) slots",
                 "bit-for-bit copy", "NaN payloads and signed zeros survive", "leave *out untouched", "do not fit i32 offsets", "wait once, for the coordinate total",
                 "do not wait at all", "t = (double)j / (double)n", "not j (1 / n)", "leaves that row unchanged", "summed in 64 bits", "-0.0 == 0.0",
                 "a NaN coordinate is never a repeat", "tolerance must be exactly 0.0", "[A, A, A, A] -> [A]", "lexicographically smallest coordinate",
                 "the closing coordinate is not a candidate", "EXACT sign of orient(u, v, w)", "not the f64 shoelace sum", "fewer than 4 coordinates",
                 "gpk_validity accepts, s is the ring's orientation", "identical at any placement and on every schedule"):
        assert line in flat, line


def test_bad_arguments_are_refused_by_the_library_before_any_device_work():
    """a NULL column or out; a scalar bound that is 0, negative or NaN; an unknown space of the per-row array; a tolerance that is not
    0; an exterior_cw that is not 0 or 1: refused with *out untouched, on a machine without a GPU too.  (A handle is never dereferenced
    before these checks: 64 stands in for one.)"""
    lib = _abi.lib()
    fake = C.c_void_p(64)
    per_row = np.ones(4)

    def refused(name, call):
        for a, with_out in ((None, True), (fake, False)):
            out = C.c_void_p(7)
            assert call(a, C.byref(out) if with_out else None) == _abi.GPK_ERR_INVALID_ARGUMENT and name in _abi.last_error()
            assert out.value == 7

    refused("segmentize", lambda a, out: lib.gpk_segmentize(a, 1.0, None, _abi.MEM_HOST, None, out))
    refused("remove_repeated_points", lambda a, out: lib.gpk_remove_repeated_points(a, 0.0, None, out))
    refused("reverse", lambda a, out: lib.gpk_reverse(a, None, out))
    refused("orient_polygons", lambda a, out: lib.gpk_orient_polygons(a, 0, None, out))
    for call, name in [(lambda out, m=m: lib.gpk_segmentize(fake, m, None, _abi.MEM_HOST, None, out), "segmentize") for m in (0.0, -1.0, float("nan"), -0.0)] + \
                      [(lambda out, sp=sp: lib.gpk_segmentize(fake, 1.0, per_row.ctypes.data, sp, None, out), "segmentize") for sp in (7, -1)] + \
                      [(lambda out, t=t: lib.gpk_remove_repeated_points(fake, t, None, out), "remove_repeated_points") for t in (1e-9, -1.0, float("nan"), float("inf"))] + \
                      [(lambda out, cw=cw: lib.gpk_orient_polygons(fake, cw, None, out), "orient_polygons") for cw in (2, -1, 256)]:
        out = C.c_void_p(7)
        assert call(C.byref(out)) == _abi.GPK_ERR_INVALID_ARGUMENT and name in _abi.last_error()
        assert out.value == 7


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(_abi.GeopolarsHipError) as e:
        call()
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_the_four_methods_check_their_arguments_before_the_device(no_device):
    s = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 2.0), (3.0, 3.0)], [(0.0, 0.0), (5.0, 0.0)]]))
    for call in (
        lambda: s.segmentize([1.0, 2.0]),  # one value per row
        lambda: s.segmentize([[1.0, 2.0, 3.0]]),
        lambda: s.segmentize("1.0"),
        lambda: s.segmentize(["a", "b", "c"]),
        lambda: s.segmentize(None),
        lambda: s.segmentize(True),
        lambda: s.segmentize(0.0),
        lambda: s.segmentize(-2),
        lambda: s.segmentize(float("nan")),
        lambda: s.remove_repeated_points(1e-9),
        lambda: s.remove_repeated_points(-1.0),
        lambda: s.remove_repeated_points(float("nan")),
        lambda: s.remove_repeated_points("0"),
        lambda: s.orient_polygons(1),
        lambda: s.orient_polygons(0),
        lambda: s.orient_polygons(None),
        lambda: s.orient_polygons("yes"),
    ):
        _refused(call)
    assert s._dev is None
