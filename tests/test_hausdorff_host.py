"""Hausdorff and Frechet distance, host side: the kernels' rules (csrc/gpk_hausdorff.h, csrc/gpk_frechet.h) run on the CPU by a
stand-alone program with the lane groups emulated, against the exact fixture — plain and under AddressSanitizer + UBSan, at the lattice
and at the georeferenced placements — and the checks that need no device: the C ABI symbols, and the Python refusals that come before
the library is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import FRECHET_MAX_SHORT, MAX_SUBDIVISIONS, GeoSeries, densify_arg, distance_rows_arg
from tests import exact_ref as X
from tests import hausdorff_ref as H
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KS = (1, 2, 3, 7)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "hausdorff", fp_contract_off=True)


@pytest.fixture(scope="module")
def exact():
    """{(placement, k): (pairs, [(H, bound)], [F^2 or None])}, computed once for both builds"""
    z = np.load(H.GOLDEN)
    out = {}
    for name, off in [("lattice", (0.0, 0.0))] + [(f"placement_{i}", p) for i, p in enumerate(X.PLACEMENTS)]:
        pairs = H.load_pairs(z, off)
        for k in KS:
            hs = [H.hausdorff_rowwise(ka, [ra], kb, [rb], k)[0] for _, ka, ra, kb, rb in pairs]
            fs = [H.frechet_exact(ra, rb, k) if ka == H.LS and kb == H.LS else None for _, ka, ra, kb, rb in pairs]
            out[(name, k)] = (pairs, hs, fs)
    return out


def _run_driver(exe, workdir, pairs, k):
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    with open(fin, "wb") as f:
        f.write(H.driver_records(pairs, k))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.fromfile(fout, dtype=np.float64).reshape(-1, 6)
    assert len(got) == len(pairs)
    return got


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, exact, build):
    """every fixture pair at the lattice and the six georeferenced placements, k in {1, 2, 3, 7}: the Hausdorff distance by 8 lanes, by 32
    lanes and by the work-group fold within 16 u (H + 2 lmax) of the exact value and bit-identical to each other; the Frechet distance
    by 8, 32 and 64 lanes within 4 u relative and bit-identical; both also with the sides exchanged"""
    built, workdir = drivers
    worst_h = worst_f = 0.0
    for (place, k), (pairs, hs, fs) in exact.items():
        got = _run_driver(built[build], workdir, pairs, k)
        back = _run_driver(built[build], workdir, [(n, kb, rb, ka, ra) for n, ka, ra, kb, rb in pairs], k)
        assert got.tobytes() == back.tobytes(), (place, k)
        for i, (name, ka, ra, kb, rb) in enumerate(pairs):
            for v in range(3):
                worst_h = max(worst_h, H.check_hausdorff(got[i, v:v + 1], [hs[i]], (place, k, name, v)))
            assert got[i, 0].tobytes() == got[i, 1].tobytes() == got[i, 2].tobytes(), (place, k, name)
            if ka == H.LS and kb == H.LS:
                for v in range(3, 6):
                    worst_f = max(worst_f, H.check_frechet(got[i, v], fs[i], (place, k, name, v)))
                assert got[i, 3].tobytes() == got[i, 4].tobytes() == got[i, 5].tobytes(), (place, k, name)
            else:
                assert np.isnan(got[i, 3:]).all()
    print(f"worst error: Hausdorff {worst_h:.3g} of 16 u (H + 2 lmax), Frechet {worst_f:.3g} of 4 u F")
    assert worst_h <= 1.0 and worst_f <= 1.0


def test_host_driver_known_answers(drivers):
    built, workdir = drivers
    pairs = list(H.KNOWN)
    names = [p[0] for p in pairs]
    k1, k2 = _run_driver(built["plain"], workdir, pairs, 1), _run_driver(built["plain"], workdir, pairs, 2)
    at = names.index
    assert k1[at("postgis_1"), 0] == 14.142135623730951 and k2[at("postgis_1"), 0] == 70.0 and k1[at("jts_1"), 0] == 22.360679774997898
    assert k1[at("frechet_doc"), 3] == 70.71067811865476 and k2[at("frechet_doc"), 3] == 50.0
    assert k1[at("reversed"), 3] == 10.0 and k1[at("reversed"), 0] == 0.0 and k1[at("identical"), 0] == 0.0 and not np.signbit(k1[at("identical"), 0])
    assert k1[at("directed"), 0] == 4.123105625617661


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_documented():
    exported = exported_symbols()
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, n_args in (("gpk_hausdorff_distance", 7), ("gpk_frechet_distance", 8)):
        assert name in _abi.EXPORTED_SYMBOLS and len(_abi._PROTOS[name][1]) == n_args and name in exported and name in doc
    assert ("int32_t gpk_hausdorff_distance(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, int32_t subdivisions, double* out, "
            "int32_t out_space, void* stream);") in flat
    assert ("int32_t gpk_frechet_distance(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, int32_t subdivisions, double* out, "
            "int64_t* n_over, int32_t out_space, void* stream);") in flat
    assert f"#define GPK_MAX_SUBDIVISIONS {MAX_SUBDIVISIONS}" in flat and MAX_SUBDIVISIONS == H.MAX_SUBDIVISIONS == 4096
    assert f"#define GPK_FRECHET_MAX_SHORT {FRECHET_MAX_SHORT}" in flat and FRECHET_MAX_SHORT == H.FRECHET_MAX_SHORT >= 4096
    for line in ("p_i.x + (double)j * ((p_(i+1).x - p_i.x) / (double)k)", "16 u (H + 2 lmax)", "relative error at most 4 u", "ONE ordered sequence per side",
                 "two identical rows give exactly 0.0", "bit-identical"):
        assert line in flat, line
    srcs = "".join(open(os.path.join(ROOT, "geopolars_amd", "csrc", f)).read() for f in ("gpk_frac.h", "gpk_hausdorff.h", "gpk_hausdorff.hip", "gpk_frechet.h", "gpk_frechet.hip"))
    assert "HD_LARGE_COST = PD_LARGE_COST" in srcs and "FR_LARGE_COST = 1 << 14" in srcs and H.FR_LARGE_COST == 1 << 14 and H.HD_LARGE_COST == 1 << 16


def test_null_and_out_of_range_arguments_are_refused_before_any_device_work():
    lib = _abi.lib()
    out = (C.c_double * 1)()
    assert lib.gpk_hausdorff_distance(None, None, None, 1, out, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert lib.gpk_frechet_distance(None, None, None, 1, out, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert "NULL" in _abi.last_error()


# ---- Python: refusals before the library is opened ----------------------------------------------------------------------------------
def test_densify_to_k_and_its_errors(no_device):
    assert [densify_arg("op", d) for d in (None, 1, 1.0, 0.5, 0.25, 1 / 3, 1 / 7, 0.4, 1 / 4096)] == [1, 1, 1, 2, 4, 3, 7, 2, 4096]
    assert all(densify_arg("op", d) == H.densify_k(d) for d in (0.9, 0.6, 0.35, 0.2, 0.13, 0.01, 0.003))
    s = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)]]))
    for bad in (0, 0.0, -0.5, 1.5, float("nan"), float("inf"), 1 / 4097, 1e-300, "half", True):
        with pytest.raises(ValueError):
            densify_arg("op", bad)
        with pytest.raises(ValueError):
            s.hausdorff_distance(s, densify=bad)
        with pytest.raises(ValueError):
            s.frechet_distance(s, densify=bad)
    with pytest.raises(ValueError):
        s.frechet_distance(s, errors="ignore")


def test_bad_pairings_come_before_the_device(no_device):
    one = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)]]))
    two = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 2.0)]]))
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0]]))
    for op in (one.hausdorff_distance, one.frechet_distance):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            op(two)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
        for rows in ([0, 1], [[0]], "x", [-1]):
            with pytest.raises(_abi.GeopolarsHipError) as e:
                op(two, other_rows=rows)
            assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    with pytest.raises(_abi.MismatchedGeometry):
        one.frechet_distance(pts)
    with pytest.raises(_abi.MismatchedGeometry):
        pts.frechet_distance(one)
    assert distance_rows_arg("op", two, one, [0, 0]).dtype == np.uint32 and distance_rows_arg("op", one, one, None) is None
