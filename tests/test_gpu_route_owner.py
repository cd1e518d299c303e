"""The routing image's block words (csrc/gpk_route.h) in the one-launch point join: a word covers 8 x 4 raster cells and names the block's
OWNER part, and a point of an `own` cell takes its polygon from the word instead of gathering the cell's level-1 word.  Every comparison
is bit-exact (counts, sorted pairs, total) against the CPU oracle; every case asserts through gpk_index_describe that the index has a
routing image and that the path under test ran (out[5] = `own` cells > 0), and where it says so that gathers remain (out[6] - out[5] > 0:
strictly-inside cells the owner does not cover).  The level-1 table keeps every word, so GPK_TILE_KERNEL=chain (which reads it) is the
independent second answer on the same inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from geopolars_amd import synth
from tests import route_owner_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 200_003  # no multiple of 512: a ragged last tile


def test_two_owners_in_a_block(gpk, oracle):
    """40 x 40 squares, R = 256: every block with interior cells holds cells of two squares — the owner's are `own`, the other's keep the
    gather.  Left side: uniform points, block borders, the extent's maximum edges, points outside, NaN and null rows, a ragged tail,
    left_row_base != 0."""
    polys = K.grid_polygons()
    assert len(polys) == 1600 and polys.n_coords == 8000
    pts = K.left_side(polys, 256, N_ROWS, seed=5)
    out, ec, ep = K.check(oracle, pts, polys, 256, base=3_000_001, gathers_remain=True)
    assert ec.max() == 1 and len(ep) > N_ROWS // 4
    K.check(oracle, pts, polys, 256, base=0, gathers_remain=True, pred="within")


_SIZES_PROG = (
    "import numpy as np\n"
    "from oracle import pyoracle\n"
    "from tests import route_owner_cases as K\n"
    "pyoracle.build()\n"
    "polys = K.grid_polygons()\n"
    f"pts = K.left_side(polys, 256, {N_ROWS}, seed=5)\n"
    "for base in (0, 3_000_001):\n"
    "    out, ec, ep = K.check(pyoracle, pts, polys, 256, base=base, gathers_remain=True)\n"
    "print('ok', len(ep), out[5], out[6])\n"
)


@pytest.mark.parametrize("env", [{"GPK_FLOW_P": "8"}, {"GPK_FLOW_P": "4"}, {"GPK_FLOW_P": "2"}, {"GPK_FLOW_P": "1"}, {"GPK_TILE_KERNEL": "chain"}])
def test_every_tile_size_on_the_same_inputs(gpk, oracle, env):
    """the inputs of test_two_owners_in_a_block under every forced tile size and under the chain kernel + writer (both switches are read
    once per process: each in its own interpreter, one at a time)"""
    r = subprocess.run([sys.executable, "-c", _SIZES_PROG], capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, **env))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr[-3000:]


def test_parts_are_not_geometries(gpk, oracle):
    """the squares as parts of MULTIPOLYGONs with null geometries among them: the owner is a PART, a hit names the geometry, and a null
    geometry hits nothing"""
    mp, valid = K.grid_multipolygons()
    pts = K.left_side(mp, 256, 120_001, seed=9)
    out, ec, ep = K.check(oracle, pts, mp, 256, base=77, gathers_remain=True)
    assert len(ep) > 10_000 and ep[:, 1].max() < len(mp)
    assert valid[ep[:, 1]].all() and not valid.all()
    K.check(oracle, pts, mp, 256, base=0, gathers_remain=True, pred="within")


@pytest.mark.parametrize("with_hole", [False, True])
def test_smallest_image(gpk, oracle, with_hole):
    """R = 64, nine large quadrilaterals: most non-empty cells are `own`.  With a hole in one of them only the answers are asserted: its
    cells stay on whatever path the tables give them."""
    polys = K.large_polygons(with_hole)
    pts = K.left_side(polys, 64, 60_001, seed=13)
    out, ec, ep = K.check(oracle, pts, polys, 64, base=5, counters=not with_hole)
    assert len(ep) > 20_000
    if not with_hole:
        assert 2 * out[5] > out[6] > 0, out


def test_every_interior_cell_of_the_star_polygons_is_owned(gpk, oracle):
    """the benchmark's right side at a size that runs in seconds: no block of its image holds interior cells of two polygons"""
    polys = synth.star_polygons(1000, 64)
    pts = synth.uniform_points(300_000, seed=41)
    out, ec, ep = K.check(oracle, pts, polys, 512, base=0, gathers_remain=False)
    assert len(ep) > 100_000
