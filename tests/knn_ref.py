"""Reference helpers of the k-nearest-neighbours join (gpk_knn_join): the expected result from a distance matrix, and the exact k-nearest
sets of the dwithin_ref fixtures with the rows on which an exact comparison is fair.

A left row is DECIDED at k when it has at most k usable partners (all of them are returned), or when its exact k-th and (k+1)-th
distances differ by more than 1e-6 relative — far above the distance routines' rounding, so the computed k smallest keys are the exact k
nearest rows.  An exact tie at the k-th place counts as undecided: which of the tied rows the computed doubles prefer is not the exact
reference's business.  tests/test_knn_host.py bounds the undecided rows on the CPU; the GPU test compares sets on the decided rows."""
import numpy as np

from tests import exact_ref as X

REL_GAP = 1e-6
MAX_UNDECIDED = 0.10


def expected_from_matrix(D, k, max_distance=float("inf"), exclude_self=False, left_row_base=0):
    """(pairs sorted by (l, d, r), counts, distances) of the knn join from the matrix of the library's own distances (NaN: unusable):
    per left row a stable sort of (D, r) over the non-NaN entries <= max_distance (without column l + left_row_base when
    exclude_self), the first k.  The l of a pair carries left_row_base."""
    pairs, dist, counts = [], [], np.zeros(D.shape[0], dtype=np.uint32)
    for l in range(D.shape[0]):
        row = D[l] + 0.0
        with np.errstate(invalid="ignore"):
            ok = row <= max_distance  # (false for NaN)
        if exclude_self and 0 <= l + left_row_base < D.shape[1]:
            ok[l + left_row_base] = False
        rr = np.nonzero(ok)[0]
        rr = rr[np.argsort(row[rr], kind="stable")][:k]  # (rr ascending, stable: ties go to the lower right row)
        counts[l] = len(rr)
        pairs += [(l + left_row_base, r) for r in rr]
        dist += row[rr].tolist()
    return np.array(pairs, dtype=np.uint32).reshape(-1, 2), counts, np.array(dist, dtype=np.float64)


def exact_knn(table, k):
    """{l: (set of the exact k nearest right rows, decided)} for every left row with a usable pair, from an exact table
    {(l, r): (d2 Fraction, lmax)} of tests/dwithin_ref.py"""
    rows = {}
    for (l, r), (d2, _) in table.items():
        rows.setdefault(l, []).append((d2, r))
    out = {}
    for l, entries in rows.items():
        entries.sort()
        if len(entries) <= k:
            out[l] = ({r for _, r in entries}, True)
            continue
        a2, b2 = entries[k - 1][0], entries[k][0]
        decided = False
        if a2 != b2:
            a, b = X.dec_sqrt(a2), X.dec_sqrt(b2)
            decided = float((b - a) / b) > REL_GAP
        out[l] = ({r for _, r in entries[:k]}, decided)
    return out


def more_than_k(table, k):
    """the left rows of an exact table with more than k usable partners"""
    n = {}
    for l, _ in table:
        n[l] = n.get(l, 0) + 1
    return {l for l, c in n.items() if c > k}
