"""Do two trees compile to the same device code?  Compares every kernel of every csrc/*.hip by mangled name.

    python tools/kernel_isa_compare.py build  <tree> <outdir>     # hipcc with the project's flags + resource remarks + --save-temps
    python tools/kernel_isa_compare.py report <outdir A> <outdir B>

report: the sets of kernels, each kernel's registers / scratch / LDS / occupancy / spills (-Rpass-analysis=kernel-resource-usage) and
its gfx950 ISA text (comments and the per-translation-unit ordinals of local labels removed), then a table of the kernels of
namespace gpk that changed translation unit.  Needs no GPU.
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill"]


def build(tree: str, out: str) -> None:
    from geopolars_amd import build as gbuild

    def one(src: str) -> tuple[str, int]:
        tu = os.path.splitext(os.path.basename(src))[0]
        d = os.path.join(out, tu)
        os.makedirs(d, exist_ok=True)
        cmd = [gbuild._hipcc(), *gbuild.FLAGS, "-Rpass-analysis=kernel-resource-usage", "--save-temps", "-x", "hip", "-c", src, "-o", tu + ".o"]
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True)
        with open(os.path.join(d, "remarks.txt"), "w") as f:
            f.write(r.stderr)
        return tu, r.returncode

    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        for tu, rc in ex.map(one, sorted(glob.glob(os.path.join(tree, "geopolars_amd", "csrc", "*.hip")))):
            print(tu, "ok" if rc == 0 else f"FAILED ({rc})")


def load(root: str):
    """mangled name -> {translation unit: (resource fields, normalised ISA text)}"""
    kernels: dict[str, dict[str, list]] = {}
    for tu in sorted(os.listdir(root)):
        d = os.path.join(root, tu)
        if not os.path.isfile(os.path.join(d, "remarks.txt")):
            continue
        cur = None
        for line in open(os.path.join(d, "remarks.txt"), errors="replace"):
            m = re.search(r"remark: .*Function Name: (\S+)", line)
            if m:
                cur = kernels.setdefault(m.group(1), {}).setdefault(tu, [{}, None])
                continue
            m = re.search(r"remark: \S+ +([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
            if m and cur is not None and m.group(1) in FIELDS:
                cur[0][m.group(1)] = m.group(2)
        for sf in glob.glob(os.path.join(d, "*gfx950*.s")):
            for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", open(sf).read(), re.S | re.M):
                if m.group(1) in kernels and tu in kernels[m.group(1)]:
                    body = re.sub(r"\s*;.*", "", m.group(2))  # comments name blocks by the function's ordinal in its unit (BB<k>_<n>)
                    body = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"[ \t]+", " ", body))
                    kernels[m.group(1)][tu][1] = body
    return kernels


def report(a_root: str, b_root: str) -> None:
    a, b = load(a_root), load(b_root)
    names = sorted(set(a) | set(b))
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    print(f"kernels (distinct mangled names over all translation units): A {len(a)}, B {len(b)}")
    print(f"only in A: {sorted(set(a) - set(b))}   only in B: {sorted(set(b) - set(a))}")
    both = [n for n in names if n in a and n in b]
    variants = lambda k, i: sorted({repr(v[i]) for v in k.values()})  # a header kernel is compiled in several units
    res_diff = [n for n in both if variants(a[n], 0) != variants(b[n], 0)]
    isa_diff = [n for n in both if variants(a[n], 1) != variants(b[n], 1)]
    no_isa = [n for n in both if any(v[1] is None for v in list(a[n].values()) + list(b[n].values()))]
    spills = lambda k: sorted(n for n, v in k.items() if any(f[0].get("VGPRs Spill", "0") != "0" or f[0].get("SGPRs Spill", "0") != "0" for f in v.values()))
    print(f"resource usage differs (any of {', '.join(FIELDS)}): {len(res_diff)}")
    for n in res_diff:
        print("   ", dem[n], variants(a[n], 0), "->", variants(b[n], 0))
    print(f"kernels with a register spill: A {len(spills(a))}, B {len(spills(b))}, the same kernels: {spills(a) == spills(b)}")
    print(f"ISA text differs: {len(isa_diff)}   (kernels whose ISA text was not found: {len(no_isa)})")
    for n in isa_diff:
        print("   ", dem[n])
    moved = [n for n in both if sorted(a[n]) != sorted(b[n]) and dem[n].replace("void ", "").startswith("gpk::")]
    print(f"\nkernels of namespace gpk that changed translation unit: {len(moved)}")
    print("%-44s %-10s %-14s %5s %5s %7s %6s %4s  %s" % ("kernel", "A", "B", "VGPR", "SGPR", "scratch", "LDS", "occ", "ISA"))
    for n in moved:
        tu_a, tu_b = sorted(a[n])[0], sorted(b[n])[0]
        f = b[n][tu_b][0]
        same = "identical" if n not in isa_diff and n not in no_isa else "DIFFERS"
        name = re.sub(r"\(.*", "", dem[n]).replace("void ", "")
        print("%-44s %-10s %-14s %5s %5s %7s %6s %4s  %s" % (name, tu_a, tu_b, f.get("VGPRs"), f.get("TotalSGPRs"), f.get("ScratchSize [bytes/lane]"), f.get("LDS Size [bytes/block]"), f.get("Occupancy [waves/SIMD]"), same))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "build":
        build(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]))
    elif len(sys.argv) == 4 and sys.argv[1] == "report":
        report(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
