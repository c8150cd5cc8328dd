"""Restatement of the inverted-file search over int8 rows (affnet_amd/csrc/ivf.hip, affnet_ivf_search_q8) for the tests: tests/_ivf.py's
restricted_knn for an integer matrix, in the order (d2, row) of tests/_knn_q8.py, and the three outputs of the call from two int8 arrays.  Plain
numpy, no device."""
import numpy as np

import _knn_q8 as kq


def restricted_knn_int(M, cell_of_row, probes, k, skip=(0, 0)):
    """First k candidates per row of the integer matrix M (n1, n2) in the order (d2, row), over the columns c with cell_of_row[c] among
    probes[r] (entries of -1 name no cell), columns skip[0] <= c < skip[0] + skip[1] (clipped to [0, n2)) removed: (d2 (n1,k) int32, idx (n1,k)
    int32); slots without a candidate hold (INT32_MAX, -1).  The values are M's own elements."""
    M, cell_of_row, probes = np.asarray(M), np.asarray(cell_of_row), np.asarray(probes)
    n1, n2 = M.shape
    lo, hi = min(max(skip[0], 0), n2), min(max(skip[0] + skip[1], 0), n2)
    keep = np.ones(n2, bool)
    keep[lo:hi] = False
    d2 = np.full((n1, k), kq.INT32_MAX, np.int32)
    idx = np.full((n1, k), -1, np.int32)
    for r in range(n1):
        cells = [int(c) for c in probes[r] if c >= 0]
        cols = np.nonzero(keep & np.isin(cell_of_row, cells))[0]
        o = cols[np.lexsort((cols, M[r, cols]))][:k]
        d2[r, :o.size] = M[r, o]
        idx[r, :o.size] = o
    return d2, idx


def expected(qa, qb, cell_of_row, probes, k, scale, skip=(0, 0)):
    """The three outputs of affnet_ivf_search_q8 for the int8 rows qa (queries) and qb (database, in ORIGINAL order) with these probes:
    (dist2 int32, dist float32 with +inf in unfilled slots, idx int32 = original rows)."""
    d2, idx = restricted_knn_int(kq.dist2(qa, qb), cell_of_row, probes, k, skip)
    dist = np.where(idx >= 0, kq.fdist(np.where(idx >= 0, d2, 0), scale), np.float32(np.inf)).astype(np.float32)
    return d2, dist, idx
