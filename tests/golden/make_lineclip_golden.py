"""Writes tests/golden/lineclip_lattice.npz, the fixture of gpk_line_clip: the rows of tests/lineclip_ref.py (integer lattices only),
and per mode the exact reference's parts — offsets, correctly rounded coordinates, and a tag per coordinate (a coordinate of the
line, a vertex of the polygon, or a crossing with its segment, ring edge and rational point).  The generator asserts the contract's
1e-6 gap condition for every row.  Deterministic, byte for byte:
python tests/golden/make_lineclip_golden.py [PATH]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import lineclip_ref as C  # noqa: E402


def main(path=None):
    data = C.fixture_bytes()
    with open(path or C.GOLDEN, "wb") as f:
        f.write(data)
    return data


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
