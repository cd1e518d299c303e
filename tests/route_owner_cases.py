"""Inputs of tests/test_gpu_route_owner.py: right sides whose raster gets a routing image (R <= 512) with blocks of 8 x 4 cells owned by
one part, by one of two, or by none, and left sides aimed at the block arithmetic.  A module of its own because the forced tile sizes
run in their own interpreter and must see the same inputs."""
import ctypes as C

import numpy as np

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GEOM_MULTIPOLYGON, GeoArrowArray

DOMAIN = 1000.0


def square(x, y, side):
    return [(x, y), (x + side, y), (x + side, y + side), (x, y + side)]


def grid_squares(n: int = 40, fill: float = 0.8):
    """n x n axis-parallel squares on the 1000-unit domain, side = fill * pitch, centred in their pitch cell.  40 x 40: 1600 polygons,
    8000 coordinates -> R = 256; a raster cell is 3.9 units, a block of 8 x 4 cells 31 x 16 units, a square 20: every block that holds
    interior cells sees two squares, the owner takes most of them and the other square's cells keep their gather."""
    pitch = DOMAIN / n
    side = fill * pitch
    off = 0.5 * (pitch - side)
    return [[square(i * pitch + off, j * pitch + off, side)] for j in range(n) for i in range(n)]


def grid_polygons() -> GeoArrowArray:
    return GeoArrowArray.from_polygons(grid_squares())


def grid_multipolygons():
    """the same squares as the members of 400 MULTIPOLYGONs, four parts each, from anywhere in the grid (part numbers and
    geometry numbers have nothing to do with each other), every seventh geometry null"""
    sq = grid_squares()
    n_geoms = 400
    perm = np.random.default_rng(17).permutation(len(sq))  # every square is a part of exactly one geometry
    mps = [[sq[perm[4 * g + k]] for k in range(4)] for g in range(n_geoms)]
    a = GeoArrowArray.from_multipolygons(mps)
    valid = np.arange(n_geoms) % 7 != 3
    return GeoArrowArray(GEOM_MULTIPOLYGON, a.xy, geom_offsets=a.geom_offsets, part_offsets=a.part_offsets, ring_offsets=a.ring_offsets,
                         validity=np.packbits(valid, bitorder="little")), valid


def large_polygons(with_hole: bool) -> GeoArrowArray:
    """R = 64: a 3 x 3 arrangement of large quadrilaterals (a raster cell is 16 units, a block 131 x 66, a polygon about 300), so most
    non-empty cells are strictly inside; with_hole: the middle one has a hole that covers blocks of its own"""
    polys = []
    for j in range(3):
        for i in range(3):
            x, y = 10.0 + 330.0 * i, 7.0 + 331.0 * j
            ext = [(x, y), (x + 305.0, y + 9.0), (x + 311.0, y + 301.0), (x + 4.0, y + 296.0)]
            if with_hole and i == 1 and j == 1:
                polys.append([ext, [(x + 60.0, y + 70.0), (x + 70.0, y + 250.0), (x + 240.0, y + 240.0), (x + 250.0, y + 60.0)]])
            else:
                polys.append([ext])
    return GeoArrowArray.from_polygons(polys)


def raster_of(polys: GeoArrowArray, R: int):
    """(rx0, ry0, fw, fh) of the R x R raster over the right side's extent: R - 3 cells span it, a cell and a half of margin"""
    mn, mx = polys.xy.min(axis=0), polys.xy.max(axis=0)
    fw, fh = (mx[0] - mn[0]) / (R - 3), (mx[1] - mn[1]) / (R - 3)
    return mn[0] - 1.5 * fw, mn[1] - 1.5 * fh, fw, fh


def block_border_points(polys: GeoArrowArray, R: int) -> np.ndarray:
    """corners of the raster cells along the borders of the 8 x 4 blocks (and the doubles next to them), and the centres of the cells on
    either side of those borders"""
    rx0, ry0, fw, fh = raster_of(polys, R)
    k = np.arange(R + 1, dtype=np.float64)
    bx, by = k[::8], k[::4]
    out = []
    gx, gy = np.meshgrid(rx0 + bx * fw, ry0 + k * fh)  # corners on the vertical block borders
    out.append(np.column_stack([gx.ravel(), gy.ravel()]))
    gx, gy = np.meshgrid(rx0 + k * fw, ry0 + by * fh)  # corners on the horizontal block borders
    out.append(np.column_stack([gx.ravel(), gy.ravel()]))
    corners = np.concatenate(out)
    out.append(np.nextafter(corners, -np.inf))
    out.append(np.nextafter(corners, np.inf))
    for side in (-0.5, 0.5):  # centres of the cells left / right of a vertical border, below / above a horizontal one
        gx, gy = np.meshgrid(rx0 + (bx + side) * fw, ry0 + (k[:-1] + 0.5) * fh)
        out.append(np.column_stack([gx.ravel(), gy.ravel()]))
        gx, gy = np.meshgrid(rx0 + (k[:-1] + 0.5) * fw, ry0 + (by + side) * fh)
        out.append(np.column_stack([gx.ravel(), gy.ravel()]))
    return np.concatenate(out)


def left_side(polys: GeoArrowArray, R: int, n_rows: int, seed: int) -> GeoArrowArray:
    """n_rows points (no multiple of 512): uniform ones, the block borders, the extent's maximum edges, points outside the extent, NaN
    rows and null rows — shuffled, so every tile holds some of each"""
    assert n_rows % 512 != 0
    rng = np.random.default_rng(seed)
    mn, mx = polys.xy.min(axis=0), polys.xy.max(axis=0)
    border = block_border_points(polys, R)
    if len(border) > n_rows // 2:
        border = border[rng.choice(len(border), n_rows // 2, replace=False)]
    t = rng.uniform(0.0, 1.0, 2000)
    edges = np.concatenate([np.column_stack([np.full(1000, mx[0]), mn[1] + t[:1000] * (mx[1] - mn[1])]),
                            np.column_stack([mn[0] + t[1000:] * (mx[0] - mn[0]), np.full(1000, mx[1])]), [[mx[0], mx[1]], [mn[0], mn[1]]]])
    w = mx - mn
    outside = np.concatenate([rng.uniform(mn - 3.0 * w, mx + 3.0 * w, (3000, 2)), [[1e30, 5.0], [5.0, -1e30], [-1e300, 1e300], [mx[0] + 1e-9, 500.0]]])
    outside = outside[np.any((outside < mn) | (outside > mx), axis=1)]
    n_uniform = n_rows - len(border) - len(edges) - len(outside)
    assert n_uniform > n_rows // 4
    xy = np.concatenate([rng.uniform(mn, mx, (n_uniform, 2)), border, edges, outside])
    rng.shuffle(xy)
    xy[rng.integers(0, n_rows, 500)] = np.nan
    xy[rng.integers(0, n_rows, 200), 0] = np.nan
    valid = rng.uniform(size=n_rows) > 0.05
    return GeoArrowArray.from_points(xy, validity=np.packbits(valid, bitorder="little"))


def index_counters(index):
    """gpk_index_describe's out[8] as a list: [5] = cells of the routing image in state `own`, [6] = raster cells strictly inside one part"""
    out = (C.c_int64 * 8)()
    _abi.check(_abi.lib().gpk_index_describe(index.handle, out))
    return [int(v) for v in out]


def check(oracle, pts, polys, R, base, gathers_remain=None, counters=True, pred="intersects"):
    """the join against the oracle, bit-exact (counts, sorted pairs, total); the index has a routing image, the owner path ran
    (out[5] > 0) and — gathers_remain True / False — some / no strictly-inside cells are left to the level-1 gather"""
    from geopolars_amd.geoseries import GeoSeries
    from geopolars_amd.spatial_index import SpatialIndex, join_pairs

    right = GeoSeries(polys)
    index = SpatialIndex(right)
    d = index.describe()
    assert d["route"] and d["R"] == R, d
    out = index_counters(index)
    if counters:
        assert out[5] > 0 and out[6] >= out[5], out
        if gathers_remain is True:
            assert out[6] - out[5] > 0, out
        if gathers_remain is False:
            assert out[6] == out[5], out
    ep, ec, _ = oracle.spatial_join(pts, polys, pred, mode=0)
    gp, gc = join_pairs(GeoSeries(pts), right, pred, r_index=index, left_row_base=base)
    ep = ep.copy()
    ep[:, 0] += base
    assert np.array_equal(gc, ec)
    assert len(gp) == len(ep) and int(gc.sum()) == len(ep)
    assert np.array_equal(gp, ep)
    return out, ec, ep
