"""Writes tests/golden/hausdorff_lattice.npz, the fixture of gpk_hausdorff_distance and gpk_frechet_distance: the pairs of
tests/hausdorff_ref.py (hand-made rows with known answers, then seeded integer-lattice rows of every unordered family pair) and the
exact reference's squared distances for them as integer fractions.  Python integers and fractions only; deterministic, byte for byte:
python tests/golden/make_hausdorff_golden.py [PATH]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import hausdorff_ref as H  # noqa: E402


def main(path=None):
    data = H.npz_bytes(H.build_arrays())
    with open(path or H.GOLDEN, "wb") as f:
        f.write(data)
    return data


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
