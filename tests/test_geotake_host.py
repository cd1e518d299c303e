"""Take and filter of geometry rows, host side: the header's host-callable routines (csrc/gpk_geotake.h: the source ranges of a row,
the rows of a strip, the window and its fallback, the locate step, the source address and the rebase) run on the CPU by a stand-alone
program — plain and under AddressSanitizer + UBSan — against GeoArrowArray.take for all six types, and the checks that need no device:
the C ABI symbols, the header's text, the refusals of the library that come before any device work, and the Python refusals that come
before the library is opened."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import SpatialJoinArgs, spatial_join
from tests import geotake_cases as K
from tests.second_pass import same_bits
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "geotake", fp_contract_off=False)


def _levels(a: GeoArrowArray):
    return [o for o in (a.geom_offsets, a.part_offsets, a.ring_offsets) if o is not None]


def _run_driver(exe, workdir, host: GeoArrowArray, idx):
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    levels = _levels(host)
    with open(fin, "wb") as f:
        f.write(struct.pack("<iqq", len(levels), len(host), len(idx)))
        for o in levels:
            f.write(struct.pack("<q", len(o)) + o.astype("<i4").tobytes())
        f.write(struct.pack("<q", host.n_coords) + host.xy.tobytes())
        f.write(np.asarray(idx, "<i8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(fout, "rb").read()
    at, got = 0, []
    for _ in levels:
        (n,) = struct.unpack_from("<q", raw, at)
        got.append(np.frombuffer(raw, "<i4", n, at + 8))
        at += 8 + 4 * n
    (n,) = struct.unpack_from("<q", raw, at)
    xy = np.frombuffer(raw, "<f8", 2 * n, at + 8).reshape(-1, 2)
    at += 8 + 16 * n
    in_range = np.frombuffer(raw, np.uint8, len(idx), at).astype(bool)
    assert at + len(idx) == len(raw)
    return got, xy, in_range


ALL = {**K.columns(), **K.edge_columns()}


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("name", list(ALL))
def test_host_driver_matches_the_host_take(drivers, build, name):
    """every column and hand-built shape, every index list: offsets of every level exactly, coordinates bit for bit, and which rows had
    no source row.  (The driver does not read the source's bitmap: validity is the row pass's, checked on the GPU.)"""
    built, workdir = drivers
    host = ALL[name]
    n = len(host)
    for what, idx in K.index_lists(n, seed=len(name)).items():
        want = K.expected_take(host, idx)
        got, xy, in_range = _run_driver(built[build], workdir, host, idx)
        for g, w in zip(got, _levels(want)):
            assert np.array_equal(g, w), (name, what)
        assert len(got) == len(_levels(want))
        assert same_bits(xy, want.xy), (name, what)
        assert np.array_equal(in_range, (idx >= 0) & (idx < n)), (name, what)


def test_the_hand_built_shapes_sit_on_the_strip_and_the_window():
    """what the edge columns claim about STRIP and WINDOW is what the header says and what their offsets are"""
    text = open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_geotake.h")).read()
    assert "constexpr int LANES = 256;" in text and "constexpr int PER_LANE = 4;" in text and "constexpr int WINDOW = 2048;" in text
    assert (K.STRIP, K.WINDOW) == (1024, 2048)
    e = K.edge_columns()
    ends = e["linestring strips"].geom_offsets[1:]
    assert ends[0] == 2500 and 3 * K.STRIP in ends and 4 * K.STRIP - 1 in ends and 4 * K.STRIP + 1 in ends
    assert np.count_nonzero(np.diff(e["multipoint empty run"].geom_offsets) == 0) > K.WINDOW + 2
    assert np.count_nonzero(np.diff(e["polygon empty run"].geom_offsets) == 0) > K.WINDOW + 2
    assert (np.diff(e["multipolygon zero parts"].geom_offsets) == 0).sum() >= 3 and e["multilinestring all empty"].n_coords == 0


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_exported_symbols_name_both_calls():
    assert "gpk_geoarray_take" in _abi.EXPORTED_SYMBOLS and "gpk_geoarray_filter" in _abi.EXPORTED_SYMBOLS
    assert len(_abi._PROTOS["gpk_geoarray_take"][1]) == 6 and _abi._PROTOS["gpk_geoarray_take"][1][2] is C.c_int64
    assert len(_abi._PROTOS["gpk_geoarray_filter"][1]) == 7


def test_built_library_exports_both_calls():
    from geopolars_amd import build

    names = exported_symbols()
    assert "gpk_geoarray_take" in names and "gpk_geoarray_filter" in names
    assert "gpk_geotake.hip" in build.SOURCES


def test_header_states_both_calls_and_the_contract():
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().replace(" * ", " ").split())
    assert ("int32_t gpk_geoarray_take(const gpk_geoarray* a, const int64_t* idx, int64_t n_idx, int32_t idx_space, void* stream, "
            "gpk_geoarray** out);") in flat
    assert ("int32_t gpk_geoarray_filter(const gpk_geoarray* a, const uint8_t* mask, int32_t mask_bits, int32_t mask_space, void* stream, "
            "gpk_geoarray** out, int64_t* n_kept);") in flat
    for line in ("bit for bit", "NaN payloads and signed zeros", "the children of a null source row", "gives a null row without children",
                 "(NaN, NaN)", "The call waits once", "2^31 - 1", "before anything is allocated", "mask_bits == 1 is an Arrow bitmap (LSB first)",
                 "mask_bits == 8 a byte per row", "*n_kept is always set", "never visit the host", "filter also waits once",
                 "ANDs the two bitmaps first", "the source may be freed first"):
        assert line in flat, line


def test_bad_arguments_are_refused_by_the_library_before_any_device_work():
    """a NULL column or out, a NULL idx with n_idx > 0, a negative n_idx, an unknown space; a mask of 2 or 16 bits a row: refused with
    *out = NULL, on a machine without a GPU too.  (A handle is never dereferenced before these checks: 64 stands in for one.)"""
    lib = _abi.lib()
    idx = np.zeros(4, np.int64)
    fake = C.c_void_p(64)
    for a, ix, n, space, with_out in ((None, idx.ctypes.data, 4, _abi.MEM_HOST, True), (fake, idx.ctypes.data, 4, _abi.MEM_HOST, False),
                                      (fake, None, 4, _abi.MEM_HOST, True), (fake, idx.ctypes.data, -1, _abi.MEM_HOST, True),
                                      (fake, idx.ctypes.data, 4, 7, True), (fake, idx.ctypes.data, 4, -1, True)):
        out = C.c_void_p(7)
        rc = lib.gpk_geoarray_take(a, ix, n, space, None, C.byref(out) if with_out else None)
        assert rc == _abi.GPK_ERR_INVALID_ARGUMENT and "geoarray_take" in _abi.last_error()
        assert not with_out or out.value is None
    mask = np.ones(4, np.uint8)
    for a, m, bits, space, with_out, with_kept in ((None, mask.ctypes.data, 8, _abi.MEM_HOST, True, True), (fake, mask.ctypes.data, 8, _abi.MEM_HOST, False, True),
                                                   (fake, mask.ctypes.data, 8, _abi.MEM_HOST, True, False), (fake, mask.ctypes.data, 2, _abi.MEM_HOST, True, True),
                                                   (fake, mask.ctypes.data, 16, _abi.MEM_HOST, True, True), (fake, mask.ctypes.data, 0, _abi.MEM_HOST, True, True),
                                                   (fake, mask.ctypes.data, 1, 5, True, True)):
        out, kept = C.c_void_p(7), C.c_int64(99)
        rc = lib.gpk_geoarray_filter(a, m, bits, space, None, C.byref(out) if with_out else None, C.byref(kept) if with_kept else None)
        assert rc == _abi.GPK_ERR_INVALID_ARGUMENT and "geoarray_filter" in _abi.last_error()
        assert not with_out or out.value is None
        assert not with_kept or kept.value == 0


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(_abi.GeopolarsHipError) as e:
        call()
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_take_and_filter_check_their_arguments_before_the_device(no_device):
    s = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]))
    for call in (
        lambda: s.take([[0, 1]]),  # 1-D
        lambda: s.take([0.0, 1.0]),  # integer dtype
        lambda: s.take(np.array([True, False, True])),
        lambda: s.take([0, 3]),  # [0, len)
        lambda: s.take([-1, 0]),  # -1 only with allow_null
        lambda: s.take([-2, 0], allow_null=True),  # exactly -1
        lambda: s.take([3], allow_null=True),
        lambda: s.filter([True, False]),  # one entry per row
        lambda: s.filter([[True, False, True]]),
        lambda: s.filter([1, 0, 1]),  # bool
        lambda: s[1],  # a scalar
        lambda: s[np.int64(1)],
        lambda: s["a"],
        lambda: s[np.array([0.5, 1.0])],
        lambda: s[np.array([0, 5])],
        lambda: s[np.array([True, False])],
    ):
        _refused(call)
    assert s._dev is None


def test_an_unknown_geometry_encoding_is_refused_before_any_device_work(no_device):
    import pyarrow as pa

    t = pa.table({"geometry": GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]).to_pyarrow(), "v": [1, 2]})
    assert SpatialJoinArgs().geometry_encoding == "wkb"
    _refused(lambda: spatial_join(t, t, SpatialJoinArgs(geometry_encoding="geojson")))
