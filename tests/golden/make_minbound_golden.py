"""Writes tests/golden/minbound_lattice.npz, the fixture of gpk_minimum_rotated_rectangle and gpk_minimum_bounding_circle: the rows of
tests/minbound_ref.py (integer lattices only) and the exact reference's verdict on them.  Deterministic, byte for byte:
python tests/golden/make_minbound_golden.py [PATH]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import minbound_ref as M  # noqa: E402


def main(path=None):
    data = M.npz_bytes(M.build_arrays())
    with open(path or M.GOLDEN, "wb") as f:
        f.write(data)
    return data


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
