"""Plain numpy restatement of the single-pair matcher (affnet_amd/csrc/match.hip: affnet_distance_matrix, affnet_match_snn), operation by
operation in float32, and the inputs of the tests that use it.  numpy and tests/_fp32_chain.py only: no torch, no affnet_amd, no GPU.
tests/test_match_mirror_host.py ties every function here to something the project already trusts (libm fmaf, the oracle, the float64
restatement, the golden graf pair) and proves that the inputs contain the cases they claim; tests/test_gpu_matcher.py compares the kernels
with it on the bytes.

What the kernels do, as restated here:
  sqnorm      lane l of 64 runs s = fmaf(x[l + 64 k], x[l + 64 k], s) from 0 over k, then the xor butterfly s[l] += s[l ^ o], o = 32 .. 1; lane 0
  dots        one fmaf chain from 0 per (row, column), in the order the fragments of rowmin_dist_body feed v_mfma_f32_16x16x4_f32:
              for t in 0 .. dim / 16: for j in 0 .. 3: for kq in 0 .. 3: k = 16 t + 4 kq + j  (kq is the MFMA's own K index)
  distance    sqrt(((asq + bsq) - 2 acc) + 1e-6f), every operation rounded on its own; a negative radicand gives NaN
  row minimum a NaN in front of every number, then the smaller value, then the smaller column (torch.min's rule on the CPU)
  second pass the COLUMNS of all nearest neighbours set to 100000 for every row (dist[:, idxs_in_2] = 100000), the row minimum again
  selection   md / (md2 + 1e-8f) <= thr in float32, the kept rows in row order as (row, idx[row])
"""
import itertools

import numpy as np

from _fp32_chain import F32, _round_odd_sum, fma32

MASKED = F32(100000.0)
EPS_D, EPS_R = F32(1e-6), F32(1e-8)

# affnet_distance_matrix; affnet_match_snn runs these and the four sizes around the 1024-row selection round
MATRIX_SHAPES = [(1, 1), (1, 17), (15, 16), (16, 15), (17, 33), (63, 40), (64, 64), (65, 200), (130, 1), (200, 415)]
MATCH_SHAPES = MATRIX_SHAPES + [(1023, 200), (1024, 200), (1025, 200), (2049, 200)]


def k_order(dim, natural=False):
    """The K index of every step of a dot product's chain."""
    assert dim % 16 == 0
    if natural:
        return list(range(dim))
    return [16 * t + 4 * kq + j for t in range(dim // 16) for j in range(4) for kq in range(4)]


def sqnorm(x, sequential=False):
    """(n, dim) float32 -> (n,) float32, dim a multiple of 64.  sequential: the variant s = fmaf(x[k], x[k], s) over k ascending."""
    x = np.ascontiguousarray(x, dtype=F32)
    n, dim = x.shape
    if sequential:
        s = np.zeros(n, F32)
        for k in range(dim):
            s = fma32(x[:, k], x[:, k], s)
        return s
    assert dim % 64 == 0
    s = np.zeros((n, 64), F32)
    for k in range(dim // 64):
        s = fma32(x[:, 64 * k:64 * k + 64], x[:, 64 * k:64 * k + 64], s)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
        assert s.dtype == F32
    return np.ascontiguousarray(s[:, 0])


def dots(a, b, natural=False):
    """(n1, dim), (n2, dim) float32 -> (n1, n2) float32 a.b as one fmaf chain from 0 per element, in k_order."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float64)            # always holds fp32 values
    for k in k_order(a.shape[1], natural):
        acc = _round_odd_sum(a64[:, k, None] * b64[None, :, k], acc).astype(F32).astype(np.float64)
    return acc.astype(F32)


def distance(a, b, natural=False, sequential=False):
    """affnet_distance_matrix: (n1, n2) float32."""
    asq, bsq, acc = sqnorm(a, sequential), sqnorm(b, sequential), dots(a, b, natural)
    r = ((asq[:, None] + bsq[None, :]) - F32(2.0) * acc) + EPS_D
    assert r.dtype == F32
    with np.errstate(invalid="ignore"):
        return np.sqrt(r)


def row_min(M, larger_column=False):
    """(value (n1,), column (n1,) int32) of the first element of every row in the order (NaN, value, column).  larger_column: the variant
    that takes the LAST of the tied elements."""
    M = np.asarray(M)
    n1, n2 = M.shape
    if larger_column:
        v, c = row_min(M[:, ::-1])
        return v, (n2 - 1 - c).astype(np.int32)
    nan = np.isnan(M)
    c = np.where(nan.any(1), nan.argmax(1), np.where(nan, np.inf, M).argmin(1)).astype(np.int32)     # argmax / argmin: the first occurrence
    return M[np.arange(n1), c], c


def match_from_matrix(M, thr, larger_column=False, strict=False):
    """affnet_match_snn from the distance matrix on: dict(md, idx, md2, ratio, keep, tent (count, 2) int32, count).  strict: the variant that
    keeps ratio < thr."""
    M = np.ascontiguousarray(M, dtype=F32)
    md, idx = row_min(M, larger_column)
    M2 = M.copy()
    M2[:, idx] = MASKED
    md2, _ = row_min(M2, larger_column)
    with np.errstate(invalid="ignore"):
        ratio = md / (md2 + EPS_R)
        assert ratio.dtype == F32
        keep = (ratio < F32(thr)) if strict else (ratio <= F32(thr))
    rows = np.nonzero(keep)[0]
    tent = np.stack([rows, idx[rows]], axis=1).astype(np.int32).reshape(-1, 2)
    return dict(md=md, idx=idx, md2=md2, ratio=ratio, keep=keep, tent=tent, count=int(rows.size))


def match(a, b, thr):
    """affnet_match_snn: match_from_matrix(distance(a, b), thr), with the matrix itself as entry M."""
    M = distance(a, b)
    return dict(match_from_matrix(M, thr), M=M)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# columns of the planted duplicates (n2 >= 40): 5 and 21 share lane 5 of the 16-column tile, one tile apart; 7 and 38 lie in lanes 7 and 6;
# 0, 16 (lane 0 again) and n2 - 1 (another lane at every n2 of the shapes) hold one row 16 times as long as the rest, chosen so that the fp32
# expansion of its self-distance falls below -1e-6: a query that copies it sees three NaN columns
DUP_SAME_LANE, DUP_OTHER_LANE, LONG_SAME_LANE = (5, 21), (7, 38), 16
HARD = 0.15        # noise per component of the hard queries: nearest at about 1.0, the unused columns at about 1.2 - on both sides of 0.8
_PLANTED = {}


def planted(n1, n2, self_copies=True):
    """(q (n1, 128), db (n2, 128)) float32, made once per shape and never modified.  The first half of the database rows are noisy unit
    copies (0.03 per component) of a pool of unit vectors, the rest random unit decoys that nobody is nearest to, all at permuted positions;
    a query is a copy of a pool row with noise 0.03 (passes the ratio test at 0.8) or HARD (about half of them do not), chosen per row.
    For n2 >= 40 also: db[0] is a row of length 16 and db[16] = db[n2 - 1] = db[0]; db[21] = db[5]; db[38] = db[7]; and with self_copies every 7th query is an exact
    copy of a database row (rows 0, 7, 14, 21 of columns 5, 7, 38, 21, the rest of random columns) and q[n1 - 2] = db[0].  The last query is
    a 0.03 copy of a pool row that takes no part in the duplicates, so that the last row of a shape is one the ratio test keeps."""
    key = (n1, n2, self_copies)
    if key not in _PLANTED:
        rng = np.random.default_rng(100003 * n1 + 17 * n2 + 5)
        ncopy = (n2 + 1) // 2
        pool = _unit(rng.normal(size=(ncopy, 128)))
        where = rng.permutation(n2)                                  # pool row i is copied to column where[i]; the other columns are decoys
        db = _unit(rng.normal(size=(n2, 128)))
        db[where[:ncopy]] = _unit(pool + 0.03 * rng.normal(size=(ncopy, 128)))
        src = rng.integers(0, ncopy, n1)
        noise = np.where(rng.random(n1) < 0.5, 0.03, HARD)
        if n1 > 1024:                                                # a refused and a kept row on the two sides of the first selection round's end
            noise[1023], noise[1024] = 0.3, 0.03
        plants = (0, LONG_SAME_LANE, n2 - 1) + DUP_SAME_LANE + DUP_OTHER_LANE
        if n2 >= 40:
            clean = [i for i in range(ncopy) if where[i] not in plants]
            src[n1 - 1], noise[n1 - 1] = clean[int(rng.integers(0, len(clean)))], 0.03
        q = _unit(pool[src] + noise[:, None] * rng.normal(size=(n1, 128))).astype(F32)
        db = db.astype(F32)
        if n2 >= 40:
            for _ in range(64):                              # a long row whose self-distance IS NaN in the arithmetic restated above
                db[0] = F32(16.0) * _unit(rng.normal(size=(1, 128)))[0].astype(F32)
                if np.isnan(distance(db[:1], db[:1])[0, 0]):
                    break
            db[n2 - 1] = db[0]
            db[LONG_SAME_LANE] = db[0]
            db[DUP_SAME_LANE[1]] = db[DUP_SAME_LANE[0]]
            db[DUP_OTHER_LANE[1]] = db[DUP_OTHER_LANE[0]]
            if self_copies:
                cols = rng.integers(0, n2, n1)
                cols[[0, 7, 14, 21]] = [DUP_SAME_LANE[0], DUP_OTHER_LANE[0], DUP_OTHER_LANE[1], DUP_SAME_LANE[1]]
                for i in range(0, n1 - 1, 7):
                    q[i] = db[cols[i]]
                q[n1 - 2] = db[0]
        q.setflags(write=False)
        db.setflags(write=False)
        _PLANTED[key] = (q, db)
    return _PLANTED[key]


_MIRROR = {}


def planted_mirror(n1, n2, thr=0.8):
    """match(q, db, thr) of planted(n1, n2), computed once."""
    key = (n1, n2, thr)
    if key not in _MIRROR:
        _MIRROR[key] = match(*planted(n1, n2), thr)
    return _MIRROR[key]


# ---- one v_mfma_f32_16x16x4_f32 ----------------------------------------------------------------------------------------------------
def mfma_input():
    """A (16, 4), B (4, 16) float32 for affnet_selftest_mfma: magnitudes 2^-12 .. 2^12 with full mantissas, and in rows 0 .. 5 of A products
    built to cancel: a1 = -a0 b0 / b1 (rounded) against column 0's b, so that a0 b0 + a1 b1 is a rounding residue that the order of the chain,
    and fusing or not fusing the multiply, decide."""
    rng = np.random.default_rng(4)
    mag = lambda shape: np.exp2(rng.uniform(-12.0, 12.0, shape)) * rng.choice([-1.0, 1.0], shape)
    A, B = mag((16, 4)).astype(F32), mag((4, 16)).astype(F32)
    B[:, 1] = B[:, 0] * F32(1.0000001)                 # a second column in which the same rows almost cancel
    for r in range(6):
        i, j = [(0, 1), (1, 2), (2, 3), (0, 3), (0, 2), (1, 3)][r]
        A[r, j] = -(A[r, i] * B[i, 0]) / B[j, 0]
        if r >= 3:                                          # the other two terms small against the residue's scale, not against the products
            for k in set(range(4)) - {i, j}:
                A[r, k] = F32(np.exp2(-20.0)) * A[r, i] * B[i, 0] / B[k, 0]
    return np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)


def mfma_chain(A, B, order=(0, 1, 2, 3)):
    """(16, 16): fma(a[o3], b[o3], fma(a[o2], b[o2], fma(a[o1], b[o1], fma(a[o0], b[o0], 0))))."""
    acc = np.zeros((A.shape[0], B.shape[1]), F32)
    for k in order:
        acc = fma32(A[:, k, None], B[None, k, :], acc)
    return acc


def mfma_unfused(A, B):
    """The same sum with the product rounded before the add (mul, add: two roundings per step), K ascending."""
    acc = np.zeros((A.shape[0], B.shape[1]), F32)
    for k in range(A.shape[1]):
        acc = acc + A[:, k, None] * B[None, k, :]
        assert acc.dtype == F32
    return acc


K_ORDERS = list(itertools.permutations(range(4)))
