"""What the host-side test modules (test_*_host.py) share: the stand-alone CPU builds of tests/<stem>_host_driver.cpp, plain and under
AddressSanitizer + UBSan (executables that are run directly: nothing is preloaded, nothing sanitized is loaded into Python), the symbols
the built library exports, and the fixture that fails a test once the library is opened."""
import os
import shutil
import subprocess

import pytest

from geopolars_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "geopolars_amd", "csrc")

BUILD_FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def compilers():
    """the host C++ compilers to try, in order: $CXX, g++, c++, clang++, ROCm's clang++ (each resolved path once)"""
    seen = []
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c) if c else None
        if p and p not in seen:
            seen.append(p)
    return seen


def build_host_drivers(tmp_path_factory, stem, fp_contract_off, builds=("plain", "sanitized")):
    """tests/<stem>_host_driver.cpp built with the host compiler, once per name in `builds` (BUILD_FLAGS), against the kernels' headers;
    `fp_contract_off` adds -ffp-contract=off, the library's own rounding contract.  Returns ({build name: executable}, the directory
    they are in)."""
    out = tmp_path_factory.mktemp(f"{stem}_driver")
    src = os.path.join(HERE, f"{stem}_host_driver.cpp")
    contract = ["-ffp-contract=off"] if fp_contract_off else []
    built = {}
    for name in builds:
        log = []
        for cxx in compilers():
            exe = str(out / f"{stem}_driver_{name}")
            r = subprocess.run([cxx, "-std=c++17", *contract, *BUILD_FLAGS[name], f"-I{CSRC}", src, "-o", exe], capture_output=True, text=True)
            if r.returncode == 0:
                built[name] = exe
                break
            log.append(f"{cxx}: {r.stderr[-400:]}")
        assert name in built, f"no host compiler built the {name} driver:\n" + "\n".join(log)
    return built, out


def exported_symbols():
    """the names the built library defines in its dynamic symbol table"""
    from geopolars_amd import build

    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture
def no_device(monkeypatch):
    """any call into the library fails the test: the checks under test must happen first"""

    def boom():
        raise AssertionError("the library was opened")

    monkeypatch.setattr(_abi, "lib", boom)
