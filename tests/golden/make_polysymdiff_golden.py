"""Writes tests/golden/polysymdiff_lattice.npz, the fixture of gpk_polygon_symdiff: the hand cases of tests/polysymdiff_ref.py, then
the input rows of tests/golden/polyunion_lattice.npz over the four family pairs — loaded from that file and compared with the rows the
reference works on, array for array — and the exact reference's result: part, ring and coordinate offsets, correctly rounded
coordinates, a tag per coordinate (an input coordinate, or a crossing with the edge of a and the edge of b that make it), and the row
status.  The generator asserts the contract's 1e-6 gap condition for every row (polysymdiff_ref.expected_columns).  Deterministic,
byte for byte:
python tests/golden/make_polysymdiff_golden.py [PATH]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import exact_ref as X  # noqa: E402
from tests import overlay_ref as O  # noqa: E402
from tests import polysymdiff_ref as S  # noqa: E402
from tests import polyunion_ref as U  # noqa: E402


def check_union_rows():
    """the rows taken over are the input rows of polyunion_lattice.npz, bit for bit"""
    z = np.load(U.GOLDEN)
    for ka, kb in U.FAMILIES:
        A, B, av, bv, _names = U.rows(ka, kb)
        for prefix, kind, rows, valid in (("a_", ka, A, av), ("b_", kb, B, bv)):
            packed = {}
            O._pack(prefix, X.column(kind, rows, valid), packed)
            for name, v in packed.items():
                w = z[U.fixture_key(ka, kb) + name]
                assert w.dtype == v.dtype and w.tobytes() == v.tobytes(), (ka, kb, name)
            assert (z[U.fixture_key(ka, kb) + prefix + "valid"] == np.array(valid, dtype=np.uint8)).all()


def main(path=None):
    check_union_rows()
    data = S.fixture_bytes()
    with open(path or S.GOLDEN, "wb") as f:
        f.write(data)
    return data


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
