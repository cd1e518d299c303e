"""Writes tests/golden/interior_lattice.npz, the fixture of gpk_representative_point: the rows of tests/interior_ref.py (integer
lattices, but for the rows whose ordinates are adjacent doubles) and the exact reference's verdict on them.  Deterministic, byte for
byte: python tests/golden/make_interior_golden.py [PATH]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import interior_ref as I  # noqa: E402


def main(path=None):
    data = I.npz_bytes(I.build_arrays())
    with open(path or I.GOLDEN, "wb") as f:
        f.write(data)
    return data


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
