"""The scratch planner, host side: the arithmetic of csrc/gpk_scratch.h (record carves, sum them, assign the slots from a base pointer)
run on the CPU by a stand-alone program — plain and under AddressSanitizer + UBSan — over a malloc'ed block that stands in for the
arena, and the checks of the source tree that need no device: nobody but the planner carves."""
import os
import re
import subprocess

import pytest

from tests.host_build import build_host_drivers

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "geopolars_amd", "csrc")


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "scratch", fp_contract_off=False)[0]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_checks_the_planner(drivers, build):
    """slots in recorded order, 256-aligned, disjoint, inside [base, base + total - SCRATCH_TAIL) and filled to their last byte;
    total = the aligned sizes + the tail; a zero-count carve has 8 bytes; a false add_if is nullptr and adds nothing; stage on the
    host, on the device and without a buffer; add_n over mixed types and both branches of stage_or_add; SCRATCH_TAIL and SCRATCH_SLOTS
    have the values the call sites were converted against; one carve beyond the capacity is a status and writes nothing; the same record twice
    gives the same offsets"""
    r = subprocess.run([drivers[build]], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert re.fullmatch(r"ok \d+\n", r.stdout), r.stdout
    assert int(r.stdout.split()[1]) > 150


def _sources():
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".h", ".hip", ".cpp")):
            yield fn, open(os.path.join(CSRC, fn)).read()


def test_only_the_planner_carves():
    """Workspace::begin and Workspace::take are private with the classes of gpk_scratch.h as their friends (the compiler's proof), no
    file but gpk_scratch.h calls them, and the three hand-kept size helpers are gone"""
    common = open(os.path.join(CSRC, "gpk_common.h")).read()
    private = common[common.index("class Workspace {"):].split("private:", 1)[1].split("};", 1)[0]
    assert "friend class Scratch;" in private and "int32_t begin(size_t" in private and "void* take(size_t" in private
    public = common[common.index("class Workspace {"):].split("private:", 1)[0]
    assert "int32_t begin(" not in public and "void* take(" not in public
    for fn, text in _sources():
        assert not re.search(r"\b(staged|clip_staging_bytes|hull_stage_bytes|take_scratch_bytes)\(", text), fn
        if fn in ("gpk_scratch.h", "gpk_runtime.hip", "gpk_common.h"):
            continue
        assert not re.search(r"(workspace\w*\([^)]*\)|\bws|\bw2?)\s*\.\s*(begin|take)\s*\(", text), fn
