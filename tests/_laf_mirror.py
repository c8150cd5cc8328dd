"""Exact fp32 mirrors of the elementwise LAF kernels of csrc/laf_ops.hip, csrc/shape_filter.h and csrc/match.hip, in numpy float32 with
fma32 (tests/_fp32_chain.py) wherever the kernel writes fmaf.  The library is built with -ffp-contract=off -fno-fast-math, and these
kernels use +, -, *, /, sqrtf and fmaf only - all correctly rounded on host and device alike - so their results are compared with
np.array_equal.  lafs2ell_kernel calls atan2f / cosf / sinf and gets a float64 restatement and a tolerance instead.

Every binary operation below is written on float32 arrays (or np.float32 scalars) so that numpy rounds it once to fp32; the asserts on
dtypes keep a silent promotion to float64 from passing as a mirror.  The decision margins are float64 recomputations from the same fp32
inputs: how far a row is from each threshold its kernel compares against."""
import numpy as np

from _fp32_chain import F32, fma32


def _f(a):
    return np.ascontiguousarray(a, dtype=F32)


def _mul22(M, L):
    """(n, 4) 2x2 matrices times the 2x2 part of (n, 2, 3) frames, bmm row by column, k ascending, fused accumulate:
    O[r][c] = fma(M[r][1], L[1][c], M[r][0] * L[0][c]); the centre column passes through."""
    M, L = _f(M).reshape(-1, 4), _f(L).reshape(-1, 2, 3)
    O = L.copy()
    O[:, 0, 0] = fma32(M[:, 1], L[:, 1, 0], M[:, 0] * L[:, 0, 0]); O[:, 0, 1] = fma32(M[:, 1], L[:, 1, 1], M[:, 0] * L[:, 0, 1])
    O[:, 1, 0] = fma32(M[:, 3], L[:, 1, 0], M[:, 2] * L[:, 0, 0]); O[:, 1, 1] = fma32(M[:, 3], L[:, 1, 1], M[:, 2] * L[:, 0, 1])
    return O


# ---- aff_shape_filter_row ------------------------------------------------------------------------------------------------------------------
_PX, _PY = (-1.0, -1.0, 1.0, 1.0), (-1.0, 1.0, -1.0, 1.0)


def eig2x2(A, sqrt=np.sqrt):
    """(l1, l2, d1) of batch_eig2x2 as the kernel writes it.  sqrt: numpy's float32 square root is correctly rounded, like the device's
    sqrtf; the host test passes torch's own (whose CPU kernel is not always) to pin every other operation bit for bit."""
    A = _f(A).reshape(-1, 4)
    a00, a01, a10, a11 = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    tr = a00 + a11
    p1, p2 = a00 * a11, a10 * a01
    d1 = tr * tr - F32(4.0) * (p1 - p2)
    mk = (d1 > 0).astype(F32)
    dl = sqrt(np.abs(d1))
    l1 = mk * (tr + dl) / F32(2.0) + F32(1000.0) * (F32(1.0) - mk)
    l2 = mk * (tr - dl) / F32(2.0) + F32(0.0001) * (F32(1.0) - mk)
    assert l1.dtype == F32 and l2.dtype == F32 and d1.dtype == F32
    return l1, l2, d1


def corners(N):
    """(n, 2, 4): the four corners (+-1, +-1) of composed frames N (n, 2, 3): fma(c, 1, fma(n_1, py, n_0 * px))."""
    N = _f(N).reshape(-1, 2, 3)
    out = np.empty((N.shape[0], 2, 4), dtype=F32)
    for k in range(4):
        px, py = F32(_PX[k]), F32(_PY[k])
        out[:, 0, k] = fma32(N[:, 0, 2], F32(1.0), fma32(N[:, 0, 1], py, N[:, 0, 0] * px))
        out[:, 1, k] = fma32(N[:, 1, 2], F32(1.0), fma32(N[:, 1, 1], py, N[:, 1, 0] * px))
    return out


def shape_filter(resp, lafs, A):
    """-> good (n,) bool, key (n,) float32, composed frames (n, 2, 3) float32."""
    resp = _f(resp).reshape(-1)
    N = _mul22(A, lafs)
    l1, l2, _ = eig2x2(A)
    with np.errstate(all="ignore"):
        ratio = np.abs(l1 / (l2 + F32(1e-8)))
    assert ratio.dtype == F32
    ok = (ratio < F32(6.0)) & (ratio > F32(1.0 / 6.0))
    c = corners(N)
    ok &= ~((c > F32(1.0)) | (c < F32(0.0))).any(axis=(1, 2))
    key = resp * ok.astype(F32)
    return ok, key, N


def shape_filter_margins(lafs, A):
    """Float64 margins of the three decisions per row: dict of (n,) arrays ratio6 = |ratio - 6|, ratio16 = |ratio - 1/6|, d1 = |d1|,
    corner = the smallest distance of a corner coordinate from 0 or 1; plus the float64 ratio, d1 and decisions themselves."""
    A = np.asarray(A, dtype=F32).astype(np.float64).reshape(-1, 4)
    L = np.asarray(lafs, dtype=F32).astype(np.float64).reshape(-1, 2, 3)
    a00, a01, a10, a11 = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    tr = a00 + a11
    d1 = tr * tr - 4.0 * (a00 * a11 - a10 * a01)
    mk = (d1 > 0).astype(np.float64)
    dl = np.sqrt(np.abs(d1))
    l1 = mk * (tr + dl) / 2.0 + 1000.0 * (1.0 - mk)
    l2 = mk * (tr - dl) / 2.0 + float(F32(0.0001)) * (1.0 - mk)
    with np.errstate(all="ignore"):
        ratio = np.abs(l1 / (l2 + float(F32(1e-8))))
    M = A.reshape(-1, 2, 2)
    N = np.concatenate([np.matmul(M, L[:, :, :2]), L[:, :, 2:]], axis=2)
    pts = np.array([_PX, _PY, (1.0, 1.0, 1.0, 1.0)])
    c = np.matmul(N, pts)
    corner = np.minimum(np.abs(c), np.abs(c - 1.0)).reshape(len(A), -1).min(axis=1)
    inside = ~((c > 1.0) | (c < 0.0)).any(axis=(1, 2))
    return {"ratio6": np.abs(ratio - 6.0), "ratio16": np.abs(ratio - float(F32(1.0 / 6.0))), "d1": np.abs(d1), "corner": corner, "ratio": ratio,
            "d1_value": d1, "inside": inside, "ratio_ok": (ratio < 6.0) & (ratio > float(F32(1.0 / 6.0)))}


def shape_filter_select(resp, lafs, ids, A, count, n_features):
    """affnet_shape_filter_select where no more than n_features rows survive: the stable compaction of the good rows among the first
    `count`.  -> (resp, composed frames, ids) of the survivors in input order."""
    count = int(count)
    ok, _, N = shape_filter(resp[:count], lafs[:count], A[:count])
    assert int(ok.sum()) <= n_features, "the mirror covers the compaction branch only"
    return _f(resp)[:count][ok], N[ok], np.asarray(ids)[:count][ok]


# ---- shape_iterate_kernel / apply_rotation_kernel / scale_lafs_kernel ---------------------------------------------------------------------------
def shape_iterate(A, base, lafs, mode):
    """-> (base after the call (n, 4), lafs_out (n, 2, 3)).  mode 1: base = A * base first."""
    base = _f(base).reshape(-1, 4).copy()
    if mode == 1:
        A = _f(A).reshape(-1, 4)
        a00, a01, a10, a11 = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
        b00, b01, b10, b11 = (base[:, k].copy() for k in range(4))
        base[:, 0] = fma32(a01, b10, a00 * b00); base[:, 1] = fma32(a01, b11, a00 * b01)
        base[:, 2] = fma32(a11, b10, a10 * b00); base[:, 3] = fma32(a11, b11, a10 * b01)
    return base, _mul22(base, lafs)


def apply_rotation(lafs, R):
    """L_2x2 <- L_2x2 * R: L[r][c] = fma(L[r][1], R[1][c], L[r][0] * R[0][c])."""
    L, R = _f(lafs).reshape(-1, 2, 3), _f(R).reshape(-1, 4)
    O = L.copy()
    O[:, 0, 0] = fma32(L[:, 0, 1], R[:, 2], L[:, 0, 0] * R[:, 0]); O[:, 0, 1] = fma32(L[:, 0, 1], R[:, 3], L[:, 0, 0] * R[:, 1])
    O[:, 1, 0] = fma32(L[:, 1, 1], R[:, 2], L[:, 1, 0] * R[:, 0]); O[:, 1, 1] = fma32(L[:, 1, 1], R[:, 3], L[:, 1, 0] * R[:, 1])
    return O


def scale_consts(w, h, inverse):
    """(c_a, c_x, c_y) as affnet_scale_lafs forms them: 1 / min in fp32, 1.0 / w and 1.0 / h as doubles stored to fp32."""
    fw, fh = F32(w), F32(h)
    m = fw if fw < fh else fh
    if inverse:
        return F32(1.0) / m, F32(1.0 / float(fw)), F32(1.0 / float(fh))
    return m, fw, fh


def _scale(L, c):
    L = _f(L).reshape(-1, 2, 3)
    O = np.empty_like(L)
    O[:, :, :2] = c[0] * L[:, :, :2]
    O[:, 0, 2] = c[1] * L[:, 0, 2]
    O[:, 1, 2] = c[2] * L[:, 1, 2]
    assert O.dtype == F32
    return O


def scale_lafs(lafs, w, h, inverse):
    return _scale(lafs, scale_consts(w, h, inverse))


# ---- aff_level_argmin + level_select_kernel ---------------------------------------------------------------------------------------------------
def frame_scale(lafs):
    """sqrtf(fabsf(q0 q4 - q1 q3) + 1e-12f) per frame."""
    L = _f(lafs).reshape(-1, 2, 3)
    with np.errstate(invalid="ignore"):
        sc = np.sqrt(np.abs(L[:, 0, 0] * L[:, 1, 1] - L[:, 0, 1] * L[:, 1, 0]) + F32(1e-12))
    assert sc.dtype == F32
    return sc


def level_argmin(lafs_px, ps, sigmas):
    """sigmas: float64 (n_oct * n_lvl,) in (octave, level) order.  fp32 scale / fp32 ps, widened; float64 distances sqrt(df * df); strict
    `<` from (inf, level 0): the first minimum wins and a NaN frame stays at level 0.  -> (best (n,), distances (n, tot))."""
    sig = np.asarray(sigmas, dtype=np.float64).reshape(-1)
    need = (frame_scale(lafs_px) / F32(ps)).astype(np.float64)
    df = sig[None, :] - need[:, None]
    with np.errstate(invalid="ignore"):
        d = np.sqrt(df * df)
    best = np.zeros(len(need), dtype=np.int64)
    bd = np.full(len(need), np.inf)
    for k in range(sig.size):
        with np.errstate(invalid="ignore"):
            m = d[:, k] < bd
        bd = np.where(m, d[:, k], bd)
        best = np.where(m, k, best)
    return best, d


def level_select(lafs_px, ps, sigmas, n_lvl, w, h):
    """-> ids (n, 3) int32 [octave, level, 0] and the re-normalised frames (n, 2, 3)."""
    best, _ = level_argmin(lafs_px, ps, sigmas)
    ids = np.stack([best // n_lvl, best % n_lvl, np.zeros_like(best)], axis=1).astype(np.int32)
    return ids, _scale(lafs_px, scale_consts(w, h, True))


def level_margin(lafs_px, ps, sigmas):
    """Float64 gap between the two smallest distances that belong to DIFFERENT sigma values.  Equal sigmas in neighbouring octaves are
    one value: the index rule decides there, not the arithmetic.  So are sigmas one float64 ulp apart (1.6 * 2^(1/3)^3 against 3.2): the
    choice between them is the float64 subtraction itself, which the mirror repeats exactly - values are grouped at 1e-9."""
    sig = np.asarray(sigmas, dtype=np.float64).reshape(-1)
    uniq = np.unique(np.round(sig, 9))
    need = (frame_scale(lafs_px) / F32(ps)).astype(np.float64)
    d = np.sort(np.abs(uniq[None, :] - need[:, None]), axis=1)
    return d[:, 1] - d[:, 0]


# ---- lafs2ell_kernel: float64 restatement --------------------------------------------------------------------------------------------------------
def lafs_to_ellipses_f64(lafs):
    """LAFs2ellT with bsvd2x2's U and singular values (LAF.py:35-51, :106-144), the kernel's formulas in float64, 1e-10 / 1e-12 included."""
    L = np.asarray(lafs, dtype=F32).astype(np.float64).reshape(-1, 2, 3)
    with np.errstate(all="ignore"):
        scale = np.sqrt((L[:, 0, 0] * L[:, 1, 1] - L[:, 0, 1] * L[:, 1, 0]) + 1e-10)
        a00, a01, a10, a11 = L[:, 0, 0] / scale, L[:, 0, 1] / scale, L[:, 1, 0] / scale, L[:, 1, 1] / scale
        su00, su01, su10, su11 = a00 * a00 + a01 * a01, a00 * a10 + a01 * a11, a10 * a00 + a11 * a01, a10 * a10 + a11 * a11
        phi = 0.5 * np.arctan2((su01 + su10) + 1e-12, (su00 - su11) + 1e-12)
        cp, sp = np.cos(phi), np.sin(phi)
        susum, dif = su00 + su11, su00 - su11
        sudif = np.sqrt((dif * dif + (4.0 * su01) * su10) + 1e-12)
        sig0, sig1 = np.sqrt((susum + sudif) / 2.0), np.sqrt((susum - sudif) / 2.0)
        w0, w1 = 1.0 / ((scale * scale) * (sig0 * sig0)), 1.0 / ((scale * scale) * (sig1 * sig1))
        m00, m01, m10, m11 = cp * w0, -sp * w1, sp * w0, cp * w1
        E = np.stack([L[:, 0, 2], L[:, 1, 2], m00 * cp + m01 * -sp, m00 * sp + m01 * cp, m10 * sp + m11 * cp], axis=1)
    return E


def ellipse_rel_err(got, want):
    """Per row: max |got - want| over (a, b, c) relative to the row's largest |coefficient| of `want`; rows where `want` is not finite
    give nan."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.abs(got[:, 2:] - want[:, 2:]).max(axis=1) / np.abs(want[:, 2:]).max(axis=1)


# ---- reproject_lafs_kernel / centre_nn_kernel ----------------------------------------------------------------------------------------------------
def reproject_lafs(lafs, H):
    L, h = _f(lafs).reshape(-1, 2, 3), _f(H).reshape(9)
    x, y, one = L[:, 0, 2], L[:, 1, 2], F32(1.0)
    X = fma32(h[2], one, fma32(h[1], y, h[0] * x))
    Y = fma32(h[5], one, fma32(h[4], y, h[3] * x))
    Z = fma32(h[8], one, fma32(h[7], y, h[6] * x))
    den = (x * h[6] + y * h[7]) + h[8]
    n1d = ((x * h[0] + y * h[1]) + h[2]) / (den * den)
    n2d = ((x * h[3] + y * h[4]) + h[5]) / (den * den)
    a = np.stack([h[0] / den - n1d * h[6], h[1] / den - n1d * h[7], h[3] / den - n2d * h[6], h[4] / den - n2d * h[7]], axis=1)
    assert a.dtype == F32
    O = _mul22(a, L)
    O[:, 0, 2] = X / Z
    O[:, 1, 2] = Y / Z
    return O


def centre_distances(query, ref):
    """(nq, nr) float32: sqrtf(fabsf((|a|^2 + |p|^2) - 2 p.a) + 1e-12f), a = reference centre, p = query centre."""
    q, r = _f(query).reshape(-1, 2, 3), _f(ref).reshape(-1, 2, 3)
    px, py, ax, ay = q[:, 0, 2][:, None], q[:, 1, 2][:, None], r[:, 0, 2][None, :], r[:, 1, 2][None, :]
    psq, asq = px * px + py * py, ax * ax + ay * ay
    dot = fma32(py, ay, px * ax)
    d = np.sqrt(np.abs((asq + psq) - F32(2.0) * dot) + F32(1e-12))
    assert d.dtype == F32
    return d


def centre_nn(query, ref):
    """-> (min_dist (nq,) float32, idx (nq,) int32), the first minimum (strict `<` over ascending j)."""
    d = centre_distances(query, ref)
    idx = np.argmin(d, axis=1)                                                 # numpy: the first occurrence of the minimum
    return d[np.arange(d.shape[0]), idx], idx.astype(np.int32)


# ---- fixtures shared by the host and the GPU test -----------------------------------------------------------------------------------------------
def ellipse_frames():
    """(frames (n, 2, 3) float32 pixel frames, kind (n,) array): 'aniso' random frames with axis ratio up to 5 and any rotation, 'iso'
    exactly isotropic diagonal frames (su00 == su11 bit for bit), 'negdet' frames of negative determinant, 'zero' zero 2x2 parts."""
    rng = np.random.RandomState(4711)
    L, kind = [], []
    for _ in range(200):
        s, r, th, ph = rng.uniform(2.0, 60.0), rng.uniform(1.0, 5.0), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        R = lambda t: np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
        M = s * R(th).dot(np.diag([np.sqrt(r), 1.0 / np.sqrt(r)])).dot(R(ph))
        L.append(np.concatenate([M, rng.uniform(0.0, 640.0, (2, 1))], axis=1)); kind.append("aniso")
    for s in (0.5, 1.0, 3.0, 7.25, 19.0, 100.0, 1e-3, 12345.0):
        L.append(np.array([[s, 0.0, 10.0 * s], [0.0, s, 7.0]])); kind.append("iso")
    for s in (1.0, 9.5, 40.0):
        L.append(np.array([[s, 0.0, 5.0], [0.0, -s, 6.0]])); kind.append("negdet")
        L.append(np.array([[0.0, s, 15.0], [s, 0.0, 16.0]])); kind.append("negdet")
    for k in range(3):
        L.append(np.array([[0.0, 0.0, 100.0 + k], [0.0, 0.0, 50.0 - k]])); kind.append("zero")
    return np.stack(L).astype(F32), np.array(kind)


def ellipse_reference_error(frames, kind):
    """The fp32 oracle (orc.lafs_to_ellipses_t, torch on the CPU) against the float64 restatement on the finite rows, relative to each
    row's largest coefficient: {kind: worst}.  The GPU test's bar is 8 x this per kind."""
    import torch
    import affnet_oracle as orc
    with np.errstate(all="ignore"):
        got = orc.lafs_to_ellipses_t(torch.from_numpy(np.ascontiguousarray(frames))).numpy()
    want = lafs_to_ellipses_f64(frames)
    err = ellipse_rel_err(got, want)
    return {k: float(err[kind == k].max()) for k in ("aniso", "iso")}, got, want


# fp32 matrices (found by a seeded random search over S diag(6 l (1 + d), l) S^-1) whose fp32 eigenvalue ratio is EXACTLY 6.0f - the
# cancellation in tr^2 - 4 det carries it there - while the float64 ratio of the same fp32 entries exceeds 6 by more than 1e-6: unambiguous
# by the margin rule, rejected by `ratio < 6.0f` and by float64 alike, accepted by a kernel that compares with `<=`
RATIO_EXACTLY_SIX = ((-1.1628470420837402, -5.592384338378906, 0.8531566262245178, 3.5186269283294678),
                     (8.764447212219238, 4.587536334991455, -11.965482711791992, -6.168920516967773),
                     (-8.18617057800293, 24.94696617126465, -3.7071495056152344, 11.164663314819336),
                     (13.949333190917969, 11.36752700805664, -12.392509460449219, -9.959081649780273))


def shape_rows(n=300, seed=77):
    """Rows for the shape filter: (resp (n,), lafs (n, 2, 3) normalised, ids (n, 3) int32, A (n, 4), group (n,) array of names).
    Planted groups, then random general matrices, all shuffled so that every row-count prefix holds some of each:
      'ratio'  matrices with eigenvalue ratio s^2 or 1 / s^2 for s^2 in {5.9, 5.99, 6.01, 6.1}: diag(s, 1/s) and its negative (ratio < 1),
               diag(1, -k), rotated (symmetric, a01 != 0) and sheared (similar, not symmetric) copies - small centred frames; and
               RATIO_EXACTLY_SIX;
      'd1'     rotations (complex eigenvalues, d1 < 0), the identity and unit shears (d1 == 0 exactly) - the 1000 / 0.0001 fallback;
      'corner' one mild shape, frames whose extreme corner lies at -1e-3, +1e-3, 1 - 1e-3, 1 + 1e-3 on each of the four sides;
      'random' I + N(0, 0.4) with random frames."""
    rng = np.random.RandomState(seed)
    A, L, grp = [], [], []
    small = np.array([[0.02, 0.0, 0.5], [0.0, 0.02, 0.5]])
    rot = lambda t: np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    for s2 in (5.9, 5.99, 6.01, 6.1, 1 / 5.9, 1 / 5.99, 1 / 6.01, 1 / 6.1):
        s = np.sqrt(s2)
        D = np.diag([s, 1.0 / s])
        S = np.array([[1.0, 0.7], [0.0, 1.0]])
        for M in (D, -D, np.diag([1.0, -s2]), rot(0.6).dot(D).dot(rot(0.6).T), -rot(2.1).dot(D).dot(rot(2.1).T), S.dot(D).dot(np.linalg.inv(S)),
                  S.T.dot(np.diag([1.0, -s2])).dot(np.linalg.inv(S.T))):
            A.append(M); L.append(small); grp.append("ratio")
    for M in RATIO_EXACTLY_SIX:
        A.append(np.array(M).reshape(2, 2)); L.append(small * np.array([[0.25, 0.25, 1.0]])); grp.append("ratio")
    for t in (0.3, 1.0, np.pi / 2, 2.0, 3.0):
        A.append(rot(t)); L.append(small); grp.append("d1")
        A.append(1.7 * rot(-t)); L.append(small); grp.append("d1")
    for M in (np.eye(2), np.array([[1.0, 0.5], [0.0, 1.0]]), np.array([[1.0, 0.0], [-2.0, 1.0]]), 2.0 * np.eye(2)):
        A.append(M); L.append(small); grp.append("d1")
    M0 = np.array([[1.2, 0.0], [0.1, 0.9]])
    ex, ey, r = 0.1 * 1.2, 0.1 * (0.1 + 0.9), 0.1
    for v in (-1e-3, 1e-3, 1.0 - 1e-3, 1.0 + 1e-3):
        for cx, cy in ((v + ex, 0.5), (v - ex, 0.5), (0.5, v + ey), (0.5, v - ey)):       # the frame's left / right / top / bottom extreme at v
            A.append(M0); L.append(np.array([[r, 0.0, cx], [0.0, r, cy]])); grp.append("corner")
    while len(A) < n:
        A.append(np.eye(2) + rng.normal(0.0, 0.4, (2, 2)))
        L.append(np.concatenate([rng.normal(0.0, 0.08, (2, 2)), rng.uniform(0.15, 0.85, (2, 1))], axis=1)); grp.append("random")
    order = rng.permutation(len(A))[:n]
    A = np.stack(A)[order].reshape(-1, 4).astype(F32)
    L = np.stack(L)[order].astype(F32)
    resp = rng.uniform(1.0, 100.0, len(order)).astype(F32)
    ids = np.stack([np.arange(len(order)) % 3, np.arange(len(order)) % 5, 1000 + np.arange(len(order))], axis=1).astype(np.int32)
    return resp, L, ids, A, np.array(grp)[order]


def shape_rows_conditions(resp, L, ids, A, grp):
    """The conditions the GPU test relies on; -> dict of figures.  No row within 1e-6 of a threshold (a d1 that is exactly zero in float64
    AND in fp32 is not near its threshold in any arithmetic: the identity and the unit shears are kept, and must be exactly that);
    accepted and rejected rows for each of the three criteria among the planted groups."""
    m = shape_filter_margins(L, A)
    ok, _, _ = shape_filter(resp, L, A)
    _, _, d1 = eig2x2(A)
    exact0 = (m["d1_value"] == 0.0) & (d1 == 0.0)
    worst = {k: float(m[k][~exact0].min() if k == "d1" else m[k].min()) for k in ("ratio6", "ratio16", "d1", "corner")}
    assert min(worst.values()) >= 1e-6, worst
    assert not ((m["d1_value"] == 0.0) ^ (d1 == 0.0)).any() and int(exact0.sum()) >= 3
    fall = m["d1_value"] <= 0
    ratio, corner, d1g = grp == "ratio", grp == "corner", grp == "d1"
    # each criterion decides rows both ways (the other two criteria passing where it accepts)
    assert (ratio & ok & (m["ratio"] > 5.0)).any() and (ratio & ~ok & (m["ratio"] > 6.0) & (m["ratio"] < 7.0)).any()
    assert (ratio & ok & (m["ratio"] < 0.2)).any() and (ratio & ~ok & (m["ratio"] < 1.0 / 6.0) & (m["ratio"] > 0.15)).any()
    assert (corner & ok).any() and (corner & ~ok).any() and m["ratio_ok"][corner].all() and (m["corner"][corner] < 2e-3).all()
    assert fall[d1g].all() and not ok[d1g].any() and (d1g & (m["d1_value"] < 0)).any() and (~fall & ok).any()
    assert np.array_equal(ok, m["inside"] & m["ratio_ok"])
    l1, l2, _ = eig2x2(A)
    six = np.abs(l1 / (l2 + F32(1e-8))) == F32(6.0)                            # the rows that tell `<` from `<=`
    assert int(six.sum()) == len(RATIO_EXACTLY_SIX) and m["inside"][six].all() and not ok[six].any() and (m["ratio"][six] > 6.0 + 1e-6).all()
    return dict(worst, rows=int(len(ok)), good=int(ok.sum()), ratio_exactly_six=int(six.sum()), d1_exactly_zero=int(exact0.sum()), general_a01=int((A[:, 1] != 0).sum()))


def level_frames(sigmas, ps, n=300, seed=5):
    """Pixel frames whose scale / ps lies (i) on every table sigma, (ii) at sigma (1 +- 1e-3), (iii) below the first and above the last,
    (iv) midway between neighbouring distinct sigmas, displaced by +- 1e-3 relative; as isotropic, rotated and anisotropic frames of that
    determinant; one NaN frame.  -> (frames (n, 2, 3) float32, target (n,) float64 scale / ps aimed at, kind (n,) of 'on' / 'near' /
    'out' / 'mid' / 'nan')."""
    sig = np.asarray(sigmas, dtype=np.float64).reshape(-1)
    uniq = np.unique(np.round(sig, 9))
    tg, kd = [], []
    for s in sig:
        tg.append(s); kd.append("on")
        tg += [s * (1 - 1e-3), s * (1 + 1e-3)]; kd += ["near", "near"]
    tg += [0.5 * sig.min(), 0.01, 1.7 * sig.max(), 1e4]; kd += ["out"] * 4
    for a, b in zip(uniq[:-1], uniq[1:]):
        tg += [0.5 * (a + b) * (1 - 1e-3), 0.5 * (a + b) * (1 + 1e-3)]; kd += ["mid", "mid"]
    rng = np.random.RandomState(seed)
    F, T, K = [], [], []
    rot = lambda t: np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    variant = 0
    while len(F) < n - 1:
        for t, k in zip(tg, kd):
            if variant == 0:
                M = np.eye(2)
            elif variant % 2:
                M = rot(rng.uniform(0, 2 * np.pi))
            else:
                a = rng.uniform(1.0, 3.0)
                M = rot(rng.uniform(0, 2 * np.pi)).dot(np.diag([a, 1.0 / a])).dot(rot(rng.uniform(0, 2 * np.pi)))
            F.append(np.concatenate([t * ps * M, rng.uniform(0.0, 64.0, (2, 1))], axis=1)); T.append(t); K.append(k)
        variant += 1
    order = rng.permutation(len(F))[:n - 1]
    F, T, K = np.stack(F)[order], np.array(T)[order], np.array(K)[order]
    nan = np.full((1, 2, 3), np.nan)
    pos = 100
    return (np.concatenate([F[:pos], nan, F[pos:]]).astype(F32), np.concatenate([T[:pos], [np.nan], T[pos:]]),
            np.concatenate([K[:pos], ["nan"], K[pos:]]))
