"""Numpy mirror of the int8 descriptor index (affnet_amd/csrc/knn_q8.hip) for the tests: the quantiser's rule in float32 arithmetic, the exact
integer squared distance, the reported float distance, and the k-nearest lists in the order (d2, database row) with skip range and unfilled
slots.  Plain numpy, no device.  Fixtures are made once from fixed seeds and never modified."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
D2_MAX = 128 * 254 * 254          # rows of all +127 against all -127


def quantize(x, scale):
    """q = clamp(rint(x * scale), -127, 127) in float32 (one multiply, round half to even), NaN -> 0, +-inf -> +-127:
    (q (n,128) int8, sq (n,) int32 = the rows' sums of q^2)."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * np.float32(scale)
    assert v.dtype == np.float32
    r = np.clip(np.rint(v), np.float32(-127), np.float32(127))
    r[np.isnan(v)] = 0
    q = r.astype(np.int8)
    return q, (q.astype(np.int64) ** 2).sum(1).astype(np.int32)


def dist2(qa, qb):
    """(n1, n2) int64: |qa[r] - qb[c]|^2 by the expansion the device uses, (sq_a + sq_b) - 2 a.b."""
    a, b = np.asarray(qa).astype(np.int64), np.asarray(qb).astype(np.int64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]) - 2 * (a @ b.T)


def fdist(d2, scale):
    """The reported distance: two correctly rounded float32 operations on the exact float32(d2)."""
    out = np.sqrt(np.asarray(d2).astype(np.float32)) / np.float32(scale)
    assert out.dtype == np.float32
    return out


def sorted_knn_int(M, k, skip=(0, 0)):
    """First k candidates per row of the integer matrix M (n1, n2) in the order (d2, row), columns skip[0] <= c < skip[0] + skip[1] (clipped to
    [0, n2)) removed: (d2 (n1,k) int32, idx (n1,k) int32); slots without a candidate hold (INT32_MAX, -1)."""
    M = np.asarray(M)
    n1, n2 = M.shape
    lo, hi = min(max(skip[0], 0), n2), min(max(skip[0] + skip[1], 0), n2)
    d2 = np.full((n1, k), INT32_MAX, np.int32)
    idx = np.full((n1, k), -1, np.int32)
    keep = np.ones(n2, bool)
    keep[lo:hi] = False
    cols = np.nonzero(keep)[0]
    for r in range(n1):
        o = cols[np.lexsort((cols, M[r, cols]))][:k]
        d2[r, :o.size] = M[r, o]
        idx[r, :o.size] = o
    return d2, idx


def expected(M, k, scale, skip=(0, 0)):
    """The three outputs of affnet_knn_q8 for the integer matrix M: (dist2 int32, dist float32 with +inf in unfilled slots, idx int32)."""
    d2, idx = sorted_knn_int(M, k, skip)
    dist = np.where(idx >= 0, fdist(np.where(idx >= 0, d2, 0), scale), np.float32(np.inf)).astype(np.float32)
    return d2, dist, idx


_RAND = {}


def random_rows(n, seed):
    """(n,128) int8 drawn uniformly from [-127, 127]: asymmetric data, so a swapped row / column map or a wrong k map cannot pass."""
    if (n, seed) not in _RAND:
        _RAND[(n, seed)] = np.random.default_rng(seed).integers(-127, 128, size=(n, 128)).astype(np.int8)
    return _RAND[(n, seed)]


def sq(q):
    return (np.asarray(q).astype(np.int64) ** 2).sum(1).astype(np.int32)
