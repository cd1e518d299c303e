"""The routing image's arithmetic, host side (csrc/gpk_route.h): route_order is a bijection of [0, R * R) for R = 64 .. 512, the block and
bit a point derives from its sub-cell coordinates are the ones of its cell, and the packed third word round-trips at its limits — run on
the CPU by a stand-alone program, plain and under AddressSanitizer + UBSan.  And what the header promises the callers of
gpk_index_describe."""
import os
import subprocess

import pytest

from tests.host_build import build_host_drivers

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "route", fp_contract_off=False)[0]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_checks_pass(drivers, build):
    r = subprocess.run([drivers[build]], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    lines = r.stdout.split("\n")
    for R in (64, 128, 256, 512):
        assert f"order R={R} ok" in lines and f"sub R={R} ok" in lines
    assert "pack ok" in lines


def test_the_header_is_host_callable_and_shared():
    """one definition for the build, the kernel and the driver: the header needs nothing but <cstdint>, and both device files use it"""
    csrc = os.path.join(ROOT, "geopolars_amd", "csrc")
    text = open(os.path.join(csrc, "gpk_route.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<cstdint>"]
    assert '#include "gpk_route.h"' in open(os.path.join(csrc, "gpk_index.h")).read()
    flow, build = open(os.path.join(csrc, "gpk_pipflow.hip")).read(), open(os.path.join(csrc, "gpk_pipindex.hip")).read()
    assert "route_block_sub(" in flow and "route_bit_sub(" in flow and "route_owner(" in flow and "route_rec0(" in flow
    assert "route_order(" in build and "route_pack(" in build
    assert "route_rank_kernel" not in build


def test_describe_documents_the_two_counters():
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().replace(" * ", " ").split())
    assert "int32_t gpk_index_describe(const gpk_index* idx, int64_t out[8]);" in flat
    assert 'cells of the routing image that name their polygon themselves ("own"' in flat
    assert "raster cells strictly inside one part" in flat
