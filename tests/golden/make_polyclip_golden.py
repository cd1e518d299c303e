"""Writes tests/golden/polyclip_lattice.npz, the fixture of gpk_polygon_clip: the rows of tests/polyclip_ref.py (integer lattices only),
and per mode the exact reference's result — part, ring and coordinate offsets, correctly rounded coordinates, a tag per coordinate (an
input coordinate, or a crossing with the edge of a and the edge of b that make it), and the row status.  The generator
asserts the contract's 1e-6 gap condition for every row and leaves a random row out that misses it.  Deterministic, byte for byte:
python tests/golden/make_polyclip_golden.py [PATH]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import polyclip_ref as C  # noqa: E402


def main(path=None):
    data = C.fixture_bytes()
    with open(path or C.GOLDEN, "wb") as f:
        f.write(data)
    return data


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
