"""Restatement of the inverted-file search (affnet_amd/csrc/ivf.hip) for the tests: the k-nearest lists over the columns of a distance matrix
whose cell is among a row's probes, in the order of tests/_knn_fp64.py (a NaN in front of every number, then the distance, then the row), and
the codebook training in float64 (the init rule, one Lloyd step, the k-means objective).  Plain numpy, no device."""
import numpy as np

import _knn_fp64 as kf


def restricted_knn(M, cell_of_row, probes, k, skip=(0, 0)):
    """First k candidates per row of the distance matrix M (n1, n2) in the order (NaN, distance, row), over the columns c with
    cell_of_row[c] among probes[r] (entries of -1 name no cell), columns skip[0] <= c < skip[0] + skip[1] (clipped to [0, n2)) removed:
    (dist (n1,k) of M's dtype, idx (n1,k) int32); slots without a candidate hold (+inf, -1).  The values are M's own elements."""
    M, cell_of_row, probes = np.asarray(M), np.asarray(cell_of_row), np.asarray(probes)
    n1, n2 = M.shape
    lo, hi = min(max(skip[0], 0), n2), min(max(skip[0] + skip[1], 0), n2)
    keep = np.ones(n2, bool)
    keep[lo:hi] = False
    dist = np.full((n1, k), np.inf, M.dtype)
    idx = np.full((n1, k), -1, np.int32)
    for r in range(n1):
        cells = [int(c) for c in probes[r] if c >= 0]
        cols = np.nonzero(keep & np.isin(cell_of_row, cells))[0]
        o = cols[kf.order(M[r, cols])][:k]
        dist[r, :o.size] = M[r, o]
        idx[r, :o.size] = o
    return dist, idx


def initial_rows(n, n_cells):
    """Centroid i starts as training row floor(i * n / n_cells)."""
    return [(i * n) // n_cells for i in range(n_cells)]


def sq_distance(x, c):
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)


def assign(x, c):
    """The nearest centroid of every row in float64, ties to the smaller cell."""
    return np.argmin(sq_distance(x, c), 1)


def cell_means(x, cells, c):
    """Float64 mean of every cell's rows; an empty cell keeps its row of c."""
    x, out = np.asarray(x, np.float64), np.array(c, np.float64)
    for j in range(out.shape[0]):
        rows = np.nonzero(np.asarray(cells) == j)[0]
        if rows.size:
            out[j] = x[rows].sum(0) / rows.size
    return out


def lloyd_step(x, c):
    return cell_means(x, assign(x, c), c)


def objective(x, c):
    """The k-means objective in float64: the sum over the rows of the squared distance to the nearest centroid."""
    return float(sq_distance(x, c).min(1).sum())


def layout(cells, n_cells):
    """(perm, cell_start) of an assignment: a stable sort."""
    cells = np.asarray(cells)
    perm = np.argsort(cells, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=n_cells))]).astype(np.int32)
    return perm, start
