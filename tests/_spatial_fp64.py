"""float64 restatement (numpy) of the spatial-verification rules of include/affnet_hip.h (affnet_verify_score / affnet_verify_matches), and
the planted inputs the tests of csrc/spatial.hip run on.  There is no reference implementation of this step (the reference calls cv2 /
pydegensac from notebooks only): like tests/_sift_fp64.py, this file IS the yardstick - the rules, written once more, in double precision.

Everything takes the frames already rounded to float32 (what the device sees) and computes in float64 from there."""
import numpy as np

PLANTED_H = np.array([[0.88, 0.31, -40.0], [-0.18, 0.94, 150.0], [2e-4, -1e-5, 1.0]])
CORNERS = np.array([[0.0, 0.0], [1000.0, 0.0], [1000.0, 750.0], [0.0, 750.0]])
BAND = 1e-3          # px: ten times the largest fp32-vs-fp64 difference of sqrt(e) measured on the planted inputs (1.04e-4 px)
AFFINE, HOMOGRAPHY = 0, 1


def reproject_lafs(lafs, H):
    """ReprojectionStuff.py:9-40 in float64: centre through H, 2x2 part through the local linearisation of H at the centre."""
    lafs = np.asarray(lafs, np.float64)
    x, y = lafs[:, 0, 2], lafs[:, 1, 2]
    den = x * H[2, 0] + y * H[2, 1] + H[2, 2]
    X = (x * H[0, 0] + y * H[0, 1] + H[0, 2]) / den
    Y = (x * H[1, 0] + y * H[1, 1] + H[1, 2]) / den
    lin = np.empty((len(x), 2, 2))
    lin[:, 0, 0] = H[0, 0] / den - X * H[2, 0] / den
    lin[:, 0, 1] = H[0, 1] / den - X * H[2, 1] / den
    lin[:, 1, 0] = H[1, 0] / den - Y * H[2, 0] / den
    lin[:, 1, 1] = H[1, 1] / den - Y * H[2, 1] / den
    out = np.empty_like(lafs)
    out[:, :, :2] = lin @ lafs[:, :, :2]
    out[:, 0, 2], out[:, 1, 2] = X, Y
    return out


def random_frames(rng, n):
    """Centres uniform in [50,950] x [50,700], scale 8..40 px, anisotropy 1..2, two uniform rotations."""
    c = np.stack([rng.uniform(50, 950, n), rng.uniform(50, 700, n)], 1)
    s, k = rng.uniform(8, 40, n), rng.uniform(1, 2, n)
    a, b = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    rot = lambda t: np.stack([np.stack([np.cos(t), -np.sin(t)], 1), np.stack([np.sin(t), np.cos(t)], 1)], 1)
    D = np.zeros((n, 2, 2))
    D[:, 0, 0], D[:, 1, 1] = np.sqrt(k), 1.0 / np.sqrt(k)
    L = s[:, None, None] * (rot(a) @ D @ rot(b))
    return np.concatenate([L, c[:, :, None]], 2)


def planted(T, seed, H=PLANTED_H, outlier_share=0.5):
    """-> lafs1 (T,2,3) f32, lafs2 (T,2,3) f32, tent (T,2) int32, planted (T,) bool (rows that were NOT replaced by a random frame).
    The frames of image 2 are stored in a shuffled order, so that `tent` is a real indirection."""
    rng = np.random.default_rng(seed)
    l1 = random_frames(rng, T)
    l2 = reproject_lafs(l1, H)
    l2[:, :, 2] += rng.normal(0.0, 0.3, (T, 2))
    l2[:, :, :2] *= 1.0 + 0.03 * rng.normal(0.0, 1.0, (T, 2, 2))
    out = rng.uniform(0, 1, T) < outlier_share
    fresh = random_frames(rng, T)
    l2[out] = fresh[out]
    perm = rng.permutation(T)
    l2s = np.empty_like(l2)
    l2s[perm] = l2                       # frame t of image 2 lives in row perm[t]
    tent = np.stack([np.arange(T), perm], 1).astype(np.int32)
    return l1.astype(np.float32), l2s.astype(np.float32), tent, ~out


# ---- scoring -------------------------------------------------------------------------------------------------------------------------
def gather(lafs1, lafs2, tent):
    """-> pts (T,4) float64 (NaN rows for invalid matches), M (T,2,2) float64 (NaN for invalid hypotheses), match_ok, hyp_ok."""
    lafs1, lafs2, tent = np.asarray(lafs1), np.asarray(lafs2), np.asarray(tent).reshape(-1, 2)
    T = tent.shape[0]
    i, j = tent[:, 0].astype(np.int64), tent[:, 1].astype(np.int64)
    inr = (i >= 0) & (i < len(lafs1)) & (j >= 0) & (j < len(lafs2))
    A = np.full((T, 2, 3), np.nan)
    B = np.full((T, 2, 3), np.nan)
    A[inr], B[inr] = lafs1[i[inr]].astype(np.float64), lafs2[j[inr]].astype(np.float64)
    pts = np.stack([A[:, 0, 2], A[:, 1, 2], B[:, 0, 2], B[:, 1, 2]], 1)
    match_ok = inr & np.isfinite(pts).all(1)
    pts[~match_ok] = np.nan
    a, b, c, d = A[:, 0, 0], A[:, 0, 1], A[:, 1, 0], A[:, 1, 1]
    with np.errstate(all="ignore"):
        det = a * d - b * c
        hyp_ok = match_ok & np.isfinite(A).all((1, 2)) & np.isfinite(B).all((1, 2)) & (np.abs(det) > np.float64(np.float32(1e-12)))
        inv = np.stack([np.stack([d, -b], 1), np.stack([-c, a], 1)], 1) / det[:, None, None]
        M = B[:, :, :2] @ inv
    M[~hyp_ok] = np.nan
    return pts, M, match_ok, hyp_ok


def score(lafs1, lafs2, tent, th):
    """-> dict: counts (T,) int, band (T,) int (pairs with |sqrt(e) - th| <= BAND), err (T,T) sqrt(e) with NaN for invalid pairs, hyp_ok, match_ok."""
    pts, M, match_ok, hyp_ok = gather(lafs1, lafs2, tent)
    with np.errstate(all="ignore"):
        d1 = pts[None, :, 0:2] - pts[:, None, 0:2]              # [h, t]
        d2 = pts[None, :, 2:4] - pts[:, None, 2:4]
        r = np.einsum("hij,htj->hti", M, d1) - d2
        err = np.sqrt((r * r).sum(2))
        inl = err <= th                                          # NaN -> False
        band = np.abs(err - th) <= BAND
    return {"counts": inl.sum(1).astype(np.int64), "band": band.sum(1).astype(np.int64), "err": err, "inl": inl, "hyp_ok": hyp_ok, "match_ok": match_ok,
            "pts": pts, "M": M}


def select(counts):
    """smallest h with the largest count; -1 when that count is 0."""
    counts = np.asarray(counts)
    if counts.size == 0 or counts.max() <= 0:
        return -1
    return int(np.argmax(counts))


# ---- local optimisation --------------------------------------------------------------------------------------------------------------
def _solve(A, n, tiny):
    """Gaussian elimination with partial pivoting on the augmented matrix A (n rows); None when a pivot is below tiny."""
    A = A.copy()
    m = A.shape[1]
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:n, c])))
        if not (abs(A[p, c]) >= tiny):
            return None
        if p != c:
            A[[c, p]] = A[[p, c]]
        for r in range(c + 1, n):
            A[r, c:] -= (A[r, c] / A[c, c]) * A[c, c:]
    X = np.zeros((n, m - n))
    for c in range(n - 1, -1, -1):
        X[c] = (A[c, n:] - A[c, c + 1:n] @ X[c + 1:]) / A[c, c]
    return X


def hypothesis_model(lafs1, lafs2, ij):
    A, B = np.asarray(lafs1[ij[0]], np.float64), np.asarray(lafs2[ij[1]], np.float64)
    M = B[:, :2] @ np.linalg.inv(A[:, :2])
    H = np.eye(3)
    H[:2, :2] = M
    H[:2, 2] = B[:, 2] - M @ A[:, 2]
    return H


def fit(p1, p2, model):
    """Hartley-normalised least squares on the pairs p1 -> p2; (H, None) or (None, 'degenerate')."""
    n = len(p1)
    c1, c2 = p1.sum(0) / n, p2.sum(0) / n
    m1, m2 = np.sqrt(((p1 - c1) ** 2).sum(1)).sum() / n, np.sqrt(((p2 - c2) ** 2).sum(1)).sum() / n
    if not (m1 > 0 and m2 > 0):
        return None
    s1, s2 = np.sqrt(2.0) / m1, np.sqrt(2.0) / m2
    q1, q2 = (p1 - c1) * s1, (p2 - c2) * s2
    x, y, u, v = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    one, zero = np.ones(n), np.zeros(n)
    Hn = np.eye(3)
    if model == HOMOGRAPHY:
        R = np.concatenate([np.stack([x, y, one, zero, zero, zero, -x * u, -y * u], 1), np.stack([zero, zero, zero, x, y, one, -x * v, -y * v], 1)], 0)
        rhs = np.concatenate([u, v])
        N = R.T @ R
        sol = _solve(np.concatenate([N, (R.T @ rhs)[:, None]], 1), 8, 1e-12 * np.abs(np.diag(N)).max())
        if sol is None:
            return None
        Hn = np.append(sol[:, 0], 1.0).reshape(3, 3)
    else:
        P = np.stack([x, y, one], 1)
        S = P.T @ P
        sol = _solve(np.concatenate([S, (P.T @ u)[:, None], (P.T @ v)[:, None]], 1), 3, 1e-12 * np.abs(np.diag(S)).max())
        if sol is None:
            return None
        Hn[0], Hn[1] = sol[:, 0], sol[:, 1]
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1]])
    T2i = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1]])
    H = T2i @ Hn @ T1
    with np.errstate(all="ignore"):
        if not abs(H[2, 2]) > 0:
            return None
        H = H / H[2, 2]
    return H if np.isfinite(H).all() else None


def transfer(H, pts):
    """-> sqrt of the fp64 transfer error per match (NaN for invalid matches), w."""
    with np.errstate(all="ignore"):
        w = H[2, 0] * pts[:, 0] + H[2, 1] * pts[:, 1] + H[2, 2]
        px = (H[0, 0] * pts[:, 0] + H[0, 1] * pts[:, 1] + H[0, 2]) / w - pts[:, 2]
        py = (H[1, 0] * pts[:, 0] + H[1, 1] * pts[:, 1] + H[1, 2]) / w - pts[:, 3]
        return np.sqrt(px * px + py * py), w


def refine(lafs1, lafs2, tent, th, model, lo_iters, best, start_mask, best_count=None):
    """The local optimisation from hypothesis `best` and its (fp32, i.e. the device's) inlier set `start_mask`.
    -> dict: H, mask, summary [best, best_count, n, flags], margin (smallest |sqrt(e) - th| over all pairs and refit iterations; inf when none ran)."""
    tent = np.asarray(tent).reshape(-1, 2)
    T = tent.shape[0]
    if best < 0:
        return {"H": np.eye(3), "mask": np.zeros(T, bool), "summary": [-1, 0, 0, 1], "margin": np.inf}
    pts = gather(lafs1, lafs2, tent)[0]
    cur = np.asarray(start_mask, bool).copy()
    keep_H, keep_mask, flags, margin = hypothesis_model(lafs1, lafs2, tent[best]), cur.copy(), 0, np.inf
    need = 4 if model == HOMOGRAPHY else 3
    for _ in range(lo_iters):
        if cur.sum() < need:
            flags |= 2
            break
        H = fit(pts[cur, 0:2], pts[cur, 2:4], model)
        if H is None:
            flags |= 4
            break
        err, w = transfer(H, pts)
        with np.errstate(all="ignore"):
            cur = (w > 0) & (err <= th)
            margin = min(margin, float(np.nanmin(np.abs(err - th))))
        if cur.sum() > keep_mask.sum():
            keep_H, keep_mask = H, cur.copy()
    bc = int(start_mask.sum()) if best_count is None else int(best_count)
    return {"H": keep_H, "mask": keep_mask, "summary": [int(best), bc, int(keep_mask.sum()), flags], "margin": margin}


def verify(lafs1, lafs2, tent, th=3.0, model=HOMOGRAPHY, lo_iters=3):
    """All of it in float64 (score, select, refine from the fp64 inlier set of the best hypothesis)."""
    sc = score(lafs1, lafs2, tent, th)
    best = select(sc["counts"])
    out = refine(lafs1, lafs2, tent, th, model, lo_iters, best, sc["inl"][best] if best >= 0 else None)
    out.update(counts=sc["counts"], band=sc["band"], best=best, score=sc)
    return out


def corners_through(H):
    p = np.concatenate([CORNERS, np.ones((4, 1))], 1) @ np.asarray(H, np.float64).reshape(3, 3).T
    return p[:, :2] / p[:, 2:3]


def corner_error(Ha, Hb, corners=None):
    """Largest distance between where the two models put the image corners."""
    if corners is not None:
        pa = np.concatenate([corners, np.ones((4, 1))], 1) @ np.asarray(Ha, np.float64).reshape(3, 3).T
        pb = np.concatenate([corners, np.ones((4, 1))], 1) @ np.asarray(Hb, np.float64).reshape(3, 3).T
        return float(np.sqrt(((pa[:, :2] / pa[:, 2:3] - pb[:, :2] / pb[:, 2:3]) ** 2).sum(1)).max())
    return float(np.sqrt(((corners_through(Ha) - corners_through(Hb)) ** 2).sum(1)).max())


def score_fp32(lafs1, lafs2, tent, th):
    """The device's fp32 operation sequence in numpy float32 (no fused multiply-add) -> counts, inl (T,T), sqrt(e)."""
    f = np.float32
    lafs1, lafs2, tent = np.asarray(lafs1, f), np.asarray(lafs2, f), np.asarray(tent).reshape(-1, 2)
    A, B = lafs1[tent[:, 0]], lafs2[tent[:, 1]]
    a, b, c, d = A[:, 0, 0], A[:, 0, 1], A[:, 1, 0], A[:, 1, 1]
    a2, b2, c2, d2 = B[:, 0, 0], B[:, 0, 1], B[:, 1, 0], B[:, 1, 1]
    with np.errstate(all="ignore"):
        det = a * d - b * c
        ok = np.isfinite(A).all((1, 2)) & np.isfinite(B).all((1, 2)) & (np.abs(det) > f(1e-12))
        m = np.stack([(a2 * d - b2 * c) / det, (b2 * a - a2 * b) / det, (c2 * d - d2 * c) / det, (d2 * a - c2 * b) / det], 1)
        m[~ok] = np.nan
        x1, y1, x2, y2 = A[:, 0, 2], A[:, 1, 2], B[:, 0, 2], B[:, 1, 2]
        dx, dy = x1[None, :] - x1[:, None], y1[None, :] - y1[:, None]
        u = (m[:, None, 0] * dx + m[:, None, 1] * dy) - (x2[None, :] - x2[:, None])
        v = (m[:, None, 2] * dx + m[:, None, 3] * dy) - (y2[None, :] - y2[:, None])
        e = u * u + v * v
        inl = e <= f(th) * f(th)
    return inl.sum(1), inl, np.sqrt(e.astype(np.float64))
