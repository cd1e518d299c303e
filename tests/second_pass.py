"""Helpers and the launch inventory for tests/test_gpu_second_pass.py.

Most kernels launch a capped grid (`cu_count() * k` blocks) and loop: a lane group or a work-group takes unit i, then i + groups, ...
Small fixtures give every group exactly one unit, so the loop's stride, the state a group carries from one unit to the next (LDS
lists, registers) and the barriers that make the reuse safe never run.  The helpers here size a column past the cap from the
device's CU count and fill it with a shuffled tiling of a small base column whose answers an exact reference gives.

INVENTORY lists every capped launch site of geopolars_amd/csrc — a `cu_count()` written at the launch, or a call of the shared
`group_grid` helper (gpk_common.h: 256 / G units a block, cu_count() * 32 blocks) — with the test that takes it past its cap;
tests/test_second_pass_inventory.py (no GPU) fails when a source file gains or loses a site without the list following.
FIXED_GRID_SITES lists the kernels launched on a fixed number of work-groups that loop over a device-side list, held to the sources
in the same way."""
from __future__ import annotations

import os
import re
from typing import NamedTuple, Optional

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "geopolars_amd", "csrc")
NEW = "tests/test_gpu_second_pass.py"


def second_trip_rows(cus: int, cap_mult: int, units_per_block: int, extra: Optional[int] = None) -> int:
    """a unit count past the first pass of a grid capped at cus * cap_mult blocks, with a ragged tail: one full pass plus `extra`
    units, `extra` no multiple of units_per_block.  One pass plus a handful would give only the first block a second unit; the
    default is a quarter of a pass plus 37, so that a quarter of all groups — some two thousand blocks of a cus * 32 grid at 256
    CUs — carry their state into a second unit."""
    one_pass = cus * cap_mult * units_per_block
    if extra is None:
        extra = one_pass // 4 + 37
    assert extra >= 1 and (units_per_block == 1 or extra % units_per_block != 0), (extra, units_per_block)
    n = one_pass + extra
    assert n > one_pass
    return n


def shuffled_tiling(n_base: int, n_total: int, seed: int, groups: int) -> np.ndarray:
    """`n_total` indices into range(n_base): a permutation of the base first (every base row occurs), then a seeded uniform draw.
    Not `arange % n_base`: with a periodic order and groups % n_base == 0 a group's second unit equals its first, and state left
    over from the first reproduces the right answer.  `groups` is the loop's stride in units (blocks * units per block)."""
    assert n_total >= n_base > 1 and 0 < groups < n_total
    rng = np.random.default_rng(seed)
    order = np.concatenate([rng.permutation(n_base), rng.integers(0, n_base, n_total - n_base)]).astype(np.int64)
    assert (order[:-groups] != order[groups:]).mean() >= 0.9, "too few base rows: most second units equal the first"
    return order


def rotating_tiling(n_base: int, n_total: int, groups: int) -> np.ndarray:
    """for a handful of base rows (a random draw would repeat too often): unit i is base row (i + i // groups) % n_base, so every
    unit differs from the one the same group took a trip earlier, and neighbouring groups differ too"""
    assert n_base >= 2 and 0 < groups < n_total
    i = np.arange(n_total, dtype=np.int64)
    step = 1 if (groups + 1) % n_base else 2  # (a rotation that cancels the stride would bring the same row back)
    order = (i + step * (i // groups)) % n_base
    assert (order[:-groups] != order[groups:]).all()
    return order


def first_rows(order: np.ndarray, n_base: int) -> np.ndarray:
    """the first position of every base row in `order`"""
    first = np.full(n_base, -1, dtype=np.int64)
    first[order[::-1]] = np.arange(len(order) - 1, -1, -1)
    assert (first >= 0).all()
    return first


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """float arrays equal bit for bit (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


class Site(NamedTuple):
    file: str
    kernel: str  # the kernels launched on this grid
    unit: str  # what one trip of the loop processes
    units_per_block: str
    cap_mult: Optional[int]  # blocks are capped at cu_count() * cap_mult
    occurrences: int  # how often `cu_count()` or a `group_grid` call is written at this site
    test: Optional[str]  # the test that runs the loop past its first trip; None only for an exempt site (then `note` says why)
    note: str = ""
    exempt: bool = False


INVENTORY = [
    Site("gpk_runtime.hip", "-", "-", "-", None, 1, None, "the definition of cu_count()", exempt=True),
    Site("gpk_common.h", "-", "-", "-", None, 1, None, "the declaration of cu_count()", exempt=True),
    Site("gpk_common.h", "-", "-", "-", 32, 2, None, "the definition of the shared group_grid (its name and the cu_count() it caps with): the "
         "sites that launch on it are listed below, each with its file's calls", exempt=True),
    Site("gpk_join.hip", "pip_flow (persistent point join)", "tile of points", "1", 1, 2, None,
         "one persistent work-group per CU; its tile loop is the benchmark path and runs in every point join of the suite", exempt=True),
    # ---- validity ----
    Site("gpk_validity.hip", "validity_rows_kernel<4|16, POLY>", "row", "256/G", 32, 1, f"{NEW}::test_validity_rows",
         "is_simple: test_is_simple_rows"),
    Site("gpk_validity.hip", "validity_big_kernel<POLY>", "listed row (> 512 coordinates)", "1", 8, 2, f"{NEW}::test_validity_large_rows",
         "is_simple: test_is_simple_large_rows"),
    # ---- representative point ----
    Site("gpk_interior.hip", "interior_poly_rows_kernel / interior_vertex_rows_kernel <4|16>", "row", "256/G", 32, 1,
         f"{NEW}::test_representative_point_rows"),
    Site("gpk_interior.hip", "interior_poly_big_kernel / interior_vertex_big_kernel", "listed row (> 512 coordinates)", "1", 8, 2,
         f"{NEW}::test_representative_point_large_rows"),
    # ---- relations: one group_grid serves the row-wise call and the join's refine ----
    Site("gpk_polyrel.hip", "polygon_relation_rowwise_kernel, pp refine", "row / candidate pair", "256/G", 32, 2, f"{NEW}::test_polygon_relation_rows",
         "refine: test_polygon_relation_join"),
    Site("gpk_linearea.hip", "line_polygon_relation kernels, lp refine", "row / candidate pair", "256/G", 32, 2, f"{NEW}::test_line_polygon_relation_rows",
         "refine: test_line_polygon_join"),
    Site("gpk_lineline.hip", "line_relation kernels, ll refine", "row / candidate pair", "256/G", 32, 2, f"{NEW}::test_line_relation_rows",
         "refine: test_line_relation_join"),
    Site("gpk_overlay.hip", "intersection_measure kernels, ov refine", "row / candidate pair", "256/G", 32, 2,
         f"{NEW}::test_intersection_measure_join", "the refine; row-wise: tests/test_gpu_overlay.py::test_a_million_rectangle_pairs (2^20 rows at G = 4)"),
    # ---- dwithin ----
    Site("gpk_dwithin.hip", "dwithin point / pair refine kernels (the join's refines)", "row / candidate pair", "256/G", 32, 2,
         f"{NEW}::test_dwithin_join_pair_refine", "the point refine: test_dwithin_join_point_refine (gpk_dwithin_rowwise does not launch these: it "
         "thresholds gpk_distance_rowwise)"),
    Site("gpk_dwithin.hip", "dwithin_pair_large_kernel", "listed candidate (n_A * n_B > PD_LARGE_COST)", "1", 4, 2, f"{NEW}::test_dwithin_join_large_list"),
    # ---- pair distance ----
    Site("gpk_pairdist.hip", "pairdist_kernel<8|32>", "row", "256/G", 16, 2, f"{NEW}::test_pair_distance_rows",
         "and through gpk_dwithin_rowwise: test_dwithin_rows"),
    Site("gpk_pairdist.hip", "pairdist_large_kernel", "listed row (n_A * n_B > PD_LARGE_COST)", "1", 4, 2, f"{NEW}::test_pair_distance_large_rows",
         "and through gpk_dwithin_rowwise: test_dwithin_large_rows"),
    # ---- linear referencing ----
    Site("gpk_linref.hip", "locate_point / closest_point kernels", "tile of LINREF_TILE = 2048 points", "1 tile", 16, 2,
         f"{NEW}::test_locate_and_closest_point_tiles"),
    Site("gpk_linref.hip", "interpolate_point_kernel<1|8|32>", "row", "256/G", 32, 1, f"{NEW}::test_interpolate_rows"),
    # ---- point distance ----
    Site("gpk_rowwise.hip", "point_poly_predicate / poly_poly_intersects / poly_poly_contains (group_grid)", "row", "256/G", 32, 3,
         f"{NEW}::test_polygon_predicate_rows", "points against polygons: test_point_polygon_predicate_rows"),
    Site("gpk_rowwise.hip", "distance_grouped_kernel", "128 ordered rows a wave, 4 waves", "512", 16, 1,
         f"{NEW}::test_point_distance_grouped_chunks", "also tests/test_gpu_configs.py::test_c3_full_size_every_row (a fixed 10M rows)"),
    Site("gpk_rowwise.hip", "distance_kernel<G, KIND>", "tile of DIST_TILE = 2048 points", "1 tile", 16, 2,
         f"{NEW}::test_point_distance_tiles"),
    # ---- structural, unary ----
    Site("gpk_structural.hip", "exterior_copy_kernel<4|16>", "row", "16", 16, 1, f"{NEW}::test_exterior_rows"),
    Site("gpk_unary.hip", "seq_stats_kernel (classes of 2, 8 and 16 lanes)", "sequence", "256/lanes", 16, 1, f"{NEW}::test_sequence_class_lists",
         "one launch: every length class has its own blocks, each class capped at cus * 16; the long class takes at most 4096 blocks"),
    Site("gpk_unary.hip", "affine_kernel", "coordinate", "256", 8, 1, f"{NEW}::test_affine_coordinates"),
    Site("gpk_unary.hip", "affine_rows_kernel<G>", "row", "256/G", 16, 1, f"{NEW}::test_affine_rows"),
    Site("gpk_crs.hip", "reproject kernels", "coordinate", "256", 8, 1, "tests/test_gpu_crs.py::test_grid_stride_path_is_bit_identical_per_tile"),
    Site("gpk_lineal_ops.hip", "geodesic_seq_kernel<4|16>, rdp_kernel<8|64>, rdp_compact_kernel", "sequence", "256/G", 32, 9,
         f"{NEW}::test_geodesic_length_rows", "simplify: tests/test_gpu_simplify.py::test_deep_stacks_and_a_wrapping_grid"),
    Site("gpk_wkb_device.hip", "wkb_copy_long_kernel", "listed sequence (> WKB_LONG coordinates)", "256 coordinates of one sequence", 8, 1, None,
         "cannot run at all: sequences above WKB_LONG = 4096 coordinates are listed only in the short-sequence form of the copy, which is "
         "chosen only for columns without a row above 64 coordinates; the list is always empty", exempt=True),
    # ---- joins ----
    Site("gpk_bboxjoin.hip", "pair_refine_kernel / pair_contains_kernel", "candidate pair", "16", 64, 1,
         "tests/test_gpu_predicate_instances.py::test_intersects_join_at_scale", "sized from the CU count (refine_per >= 4)"),
    Site("gpk_nearest.hip", "nearest_best_kernel / nearest_emit_kernel <1|8|32>", "left point", "256/G", 32, 2,
         f"{NEW}::test_nearest_join_rows", "also tests/test_gpu_nearest.py::test_full_size_c3_data (a fixed 10M points)"),
    # ---- convex hull ----
    Site("gpk_hull.hip", "hull_small_kernel<128, LISTED>", "listed row of 65 .. 128 points", "16", 8, 2, f"{NEW}::test_hull_mid_list"),
    Site("gpk_hull.hip", "hull_sort_big_kernel", "listed row above 128 points", "1", 8, 2, f"{NEW}::test_hull_big_list"),
    Site("gpk_hull.hip", "hull_chain_big_kernel", "listed row above 128 points, one lane each", "64", 16, 2, None,
         "left out: its own stride needs more than cus * 16 * 64 (262 144 at 256 CUs) rows above 128 points; the kernel keeps nothing "
         "between rows (registers only, scratch addressed by the row)", exempt=True),
]


class FixedSite(NamedTuple):
    file: str  # where the constant is defined
    constant: str  # the fixed number of work-groups the kernel is launched on
    kernel: str
    unit: str  # what one trip of the loop processes
    test: str  # the test that lists more units than the grid has work-groups


# Kernels on a FIXED grid (the device's CU count is not asked) that loop over a list whose length they read on the device: invisible to
# the count above, the same gap — with up to `constant` listed units every work-group takes one and the loop's second trip, with whatever
# the work-group carries in LDS from one unit to the next, never runs.
FIXED_GRID_SITES = [
    FixedSite("gpk_hausdorff.hip", "HD_LIST_BLOCKS", "hausdorff_large_kernel", "listed row (cost above HD_LARGE_COST)",
              "tests/test_gpu_hausdorff.py::test_hausdorff_list_loop_past_its_first_pass"),
    FixedSite("gpk_frechet.hip", "FR_LIST_BLOCKS", "frechet_large_kernel", "listed row (a table past the lane group's registers)",
              "tests/test_gpu_hausdorff.py::test_frechet_list_loop_past_its_first_pass"),
    FixedSite("gpk_knn.hip", "KNN_LIST_BLOCKS", "knn_select_list_kernel", "listed left row (candidates past the wave's keys)",
              "tests/test_gpu_knn.py::test_list_kernel_past_its_first_pass"),
    FixedSite("gpk_minbound.h", "MBG_BIG_BLOCKS", "the work-group kernels of gpk_minbound.hip", "listed row (a hull above MBG_SMALL_HULL vertices)",
              "tests/test_gpu_minbound.py::test_work_group_loop_second_trip"),
    FixedSite("gpk_pointrel.hip", "PT_LIST_BLOCKS", "point_relation_large_kernel", "listed unit (n_A * n_B above PT_LARGE_COST)",
              "tests/test_gpu_pointrel.py::test_list_kernel_past_its_first_pass"),
]


def counted_fixed_sites() -> dict:
    """{source file: [the fixed-grid constants it defines]} over geopolars_amd/csrc: every `constexpr ... X_LIST_BLOCKS | X_BIG_BLOCKS`"""
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(CSRC, fn)) as f:
                names = re.findall(r"constexpr\s+(?:unsigned|int)\s+(\w+_(?:LIST|BIG)_BLOCKS)\s*=", f.read())
            if names:
                out[fn] = sorted(names)
    return out


def fixed_inventory() -> dict:
    out = {}
    for s in FIXED_GRID_SITES:
        out.setdefault(s.file, []).append(s.constant)
    return {k: sorted(v) for k, v in out.items()}


def fixed_grid(constant: str) -> int:
    """the value of a fixed-grid constant, read from the source"""
    site = next(s for s in FIXED_GRID_SITES if s.constant == constant)
    with open(os.path.join(CSRC, site.file)) as f:
        return int(re.search(rf"constexpr\s+(?:unsigned|int)\s+{constant}\s*=\s*(\d+)\s*;", f.read()).group(1))


def counted_sites() -> dict:
    """{source file: number of `cu_count()` occurrences and `group_grid` calls} over geopolars_amd/csrc"""
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(CSRC, fn)) as f:
                k = len(re.findall(r"\bcu_count\(\)|\bgroup_grid\(", f.read()))
            if k:
                out[fn] = k
    return out


def inventory_counts() -> dict:
    out = {}
    for s in INVENTORY:
        out[s.file] = out.get(s.file, 0) + s.occurrences
    return out
