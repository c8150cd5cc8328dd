"""Float64 restatement of the descriptor index (affnet_amd/csrc/knn.hip) for the tests: the distance of Losses.py:5-13, the order of
candidates (a NaN in front of every number, then the distance, then the database row), the k-nearest lists with skip range and unfilled slots,
and the vote rule of affnet_knn_vote.  Plain numpy, no device."""
import numpy as np

VOTE_COUNTS = [1, 15, 16, 17, 63, 64, 65, 130, 200]


def distance(a, b):
    """sqrt((|a|^2 + |b|^2) - 2 a.b + 1e-6) in float64, (n1, n2); a negative radicand gives NaN, as on the device."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    r = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]) - 2.0 * (a @ b.T) + 1e-6
    with np.errstate(invalid="ignore"):
        return np.sqrt(r)


def order(row):
    """Indices of one row of distances in the order (NaN first, distance, index)."""
    row = np.asarray(row)
    key = np.where(np.isnan(row), -np.inf, row)
    return np.lexsort((np.arange(row.size), key))


def sorted_knn(M, k, skip=(0, 0)):
    """First k candidates per row of the distance matrix M (n1, n2) in that order, columns skip[0] <= c < skip[0] + skip[1] (clipped to
    [0, n2)) removed: (dist (n1,k) of M's dtype, idx (n1,k) int32); slots without a candidate hold (+inf, -1).  The values are M's own
    elements, bit for bit."""
    M = np.asarray(M)
    n1, n2 = M.shape
    lo, hi = min(max(skip[0], 0), n2), min(max(skip[0] + skip[1], 0), n2)
    dist = np.full((n1, k), np.inf, M.dtype)
    idx = np.full((n1, k), -1, np.int32)
    keep = np.ones(n2, bool)
    keep[lo:hi] = False
    cols = np.nonzero(keep)[0]
    for r in range(n1):
        o = cols[order(M[r, cols])][:k]
        dist[r, :o.size] = M[r, o]
        idx[r, :o.size] = o
    return dist, idx


def votes(dist, idx, ratio, row_image, n_images, dtype=np.float64):
    """affnet_knn_vote on the host in `dtype` arithmetic (one multiply, one compare per neighbour)."""
    dist, idx = np.asarray(dist).astype(dtype), np.asarray(idx)
    row_image = np.asarray(row_image)
    out = np.zeros(n_images, np.int32)
    n1, k = idx.shape
    for r in range(n1):
        bound = dtype(ratio) * dist[r, k - 1]
        voted = []
        for j in range(k - 1):
            c = int(idx[r, j])
            if not 0 <= c < row_image.size:
                continue
            img = int(row_image[c])
            if not 0 <= img < n_images or dist[r, j] > bound or img in voted:
                continue
            voted.append(img)
            out[img] += 1
    return out


def vote_margin(dist, idx, ratio):
    """Smallest |dist[r][j] - ratio * dist[r][k-1]| over the comparisons the vote rule makes (j < k-1, filled slot, finite numbers on both
    sides); +inf when it makes none."""
    dist, idx = np.asarray(dist, np.float64), np.asarray(idx)
    k = idx.shape[1]
    m = np.inf
    for j in range(k - 1):
        ok = (idx[:, j] >= 0) & np.isfinite(dist[:, j]) & np.isfinite(dist[:, k - 1])
        if ok.any():
            m = min(m, np.abs(dist[ok, j] - ratio * dist[ok, k - 1]).min())
    return m


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


_VOTE = {}


def vote_setup():
    """The images of the vote tests, made once and never modified: nine images of VOTE_COUNTS random unit descriptors (default_rng(23)), then,
    for s in (1, 3, 5, 7), a query = a permuted copy of image s with 0.005 * normal added and renormalised, plus 30 random unit rows, and last a
    tenth image for the two-copies case (a second noisy copy of image 3).  float32 arrays."""
    if not _VOTE:
        rng = np.random.default_rng(23)
        descs = [unit(rng.normal(size=(n, 128))).astype(np.float32) for n in VOTE_COUNTS]
        queries = {}
        for s in (1, 3, 5, 7):
            n = VOTE_COUNTS[s]
            q = unit(descs[s][rng.permutation(n)].astype(np.float64) + 0.005 * rng.normal(size=(n, 128)))
            queries[s] = np.concatenate([q, unit(rng.normal(size=(30, 128)))]).astype(np.float32)
        twin = unit(descs[3].astype(np.float64) + 0.005 * rng.normal(size=(VOTE_COUNTS[3], 128))).astype(np.float32)
        off = np.concatenate([[0], np.cumsum(VOTE_COUNTS)])
        _VOTE.update(descs=descs, queries=queries, twin=twin, off=off, D=np.concatenate(descs),
                     row_image=np.repeat(np.arange(len(VOTE_COUNTS)), VOTE_COUNTS).astype(np.int32))
    return _VOTE
