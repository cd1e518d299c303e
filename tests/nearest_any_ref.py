"""Reference helpers of the any-family nearest join (gpk_nearest_join_any): the expected result from a distance matrix, and the exact
argmin sets of the dwithin_ref fixtures with the rows on which an exact comparison is fair.

A left row is DECIDED when its exact best and its exact second-best distinct distances differ by more than 1e-6 relative (far above the
distance routines' rounding, so the computed minimum is taken by the exact nearest rows only), or when its best is shared exactly.
tests/test_nearest_any_host.py proves on the CPU that at most 5 % of the usable left rows of every fixture are undecided; the GPU test
compares pair sets on the decided rows."""
import numpy as np

from tests import dwithin_ref as W
from tests import exact_ref as X

# every fixture of the exact-reference GPU test, with the seed of its pair_fixture (point fixtures have none)
EXACT_FIXTURES = [(k, None) for k in W.POINT_FIXTURES] + [(k, 0) for k in W.PAIR_FIXTURES]
REL_GAP = 1e-6
MAX_UNDECIDED = 0.05


def fixture(key, seed):
    return W.point_fixture(*key) if isinstance(key[0], str) else W.pair_fixture(*key, seed=seed)


def fixture_table(key, seed):
    if seed in (None, 0):
        return W.fixture_table(key)  # (cached per process, shared with the dwithin tests)
    return W.exact_table(*fixture(key, seed))


def expected_from_matrix(D, max_distance):
    """(pairs sorted by (l, r), counts, distances) of the nearest join from the matrix of the library's own distances (NaN: unusable):
    per left row the argmin set by double equality, kept when the minimum is <= max_distance"""
    with np.errstate(invalid="ignore"):
        best = np.where(np.isnan(D).all(axis=1), np.nan, np.nanmin(np.where(np.isnan(D), np.inf, D), axis=1))
        hit = (D == best[:, None]) & (best[:, None] <= max_distance)
    ll, rr = np.nonzero(hit)
    return np.stack([ll, rr], axis=1).astype(np.uint32), np.bincount(ll, minlength=D.shape[0]).astype(np.uint32), D[ll, rr]


def exact_nearest(table, n_left):
    """{l: (sorted right rows at the exact minimum, exact squared minimum, decided, lmax of the pair at the minimum)} for every left
    row with a usable pair"""
    rows = {}
    for (l, r), (d2, lmax) in table.items():
        rows.setdefault(l, []).append((d2, r, lmax))
    out = {}
    for l, entries in rows.items():
        best = min(e[0] for e in entries)
        at = sorted(r for d2, r, _ in entries if d2 == best)
        above = [d2 for d2, _, _ in entries if d2 != best]
        decided = len(at) > 1 or not above
        if above and not decided:
            b, s = X.dec_sqrt(best), X.dec_sqrt(min(above))
            decided = float((s - b) / s) > REL_GAP
        out[l] = (at, best, decided, max(lm for d2, _, lm in entries if d2 == best))
    return out
