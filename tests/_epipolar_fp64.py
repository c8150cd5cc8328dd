"""numpy restatement of the epipolar-verification rules of include/affnet_hip.h (affnet_epipolar_score / affnet_epipolar_verify), and the
planted two-view scenes the tests of csrc/epipolar.hip run on.  There is no reference implementation of this step (the reference verifies
with cv2 / pydegensac from notebooks only): like tests/_spatial_fp64.py, this file IS the yardstick - the rules, written once more.

The hash, the members, the fp32 scoring tree and the selection are restated exactly (integers, and float32 without fused multiply-add); the
solve follows the header's operation order in float64; the refit is float64 with numpy's own summation order."""
import numpy as np

import _spatial_fp64 as sp

MAX_ROUNDS = 64
SWEEPS = 12
# px: ten times the largest difference of sqrt(e) between score_fp32 and sampson (float64) over all (hypothesis, match) pairs with an error
# below 10 px, MEASURED between these two restatements on the CPU (never on the device) on the five scenes of tests/test_epipolar_host.py
# (SCENES and PLANAR, rounds = 8, seed 0, all T * rounds hypotheses against all T matches): the largest difference was 7.51e-3 px (scene
# (500, 0.7, 8)); ten times that, rounded up to two digits.  test_band_is_ten_times_the_fp32_spread measures it again.
BAND = 7.6e-2

K = np.array([[800.0, 0.0, 500.0], [0.0, 800.0, 375.0], [0.0, 0.0, 1.0]])
ROT = np.array([[np.cos(0.25), 0.0, np.sin(0.25)], [0.0, 1.0, 0.0], [-np.sin(0.25), 0.0, np.cos(0.25)]])
TRANS = np.array([-1.5, 0.1, 0.3])
SCENES = [(200, 0.5, 7), (500, 0.7, 8), (300, 0.5, 11)]       # (T, outlier share, seed)
PLANAR = [(200, 1), (500, 2)]                                 # _spatial_fp64.planted(T, seed)


def planted_F():
    tx = np.array([[0.0, -TRANS[2], TRANS[1]], [TRANS[2], 0.0, -TRANS[0]], [-TRANS[1], TRANS[0], 0.0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ ROT @ Ki
    return F / np.sqrt((F * F).sum())


def planted_two_view(T, outlier_share, seed, frames1=None):
    """Two views of a scene with depth -> lafs1 (T,2,3) f32, lafs2 (T,2,3) f32, tent (T,2) int32, planted (T,) bool, F (3,3) with x2^T F x1 = 0.
    Every point has its own depth in [4,10] and lies on its own plane, tilted by up to 0.8 rad against the first camera's image plane; its
    frame in image 2 is its frame in image 1 pushed through that plane's homography K (R + t n^T / d) K^-1.  frames1: the frames of image 1
    to use instead of random ones."""
    rng = np.random.default_rng(seed)
    l1 = sp.random_frames(rng, T) if frames1 is None else np.asarray(frames1, np.float64)
    depth, tilt, phi = rng.uniform(4.0, 10.0, T), rng.uniform(0.0, 0.8, T), rng.uniform(0.0, 2 * np.pi, T)
    Ki = np.linalg.inv(K)
    l2 = np.empty_like(l1)
    for i in range(T):
        X = depth[i] * (Ki @ np.array([l1[i, 0, 2], l1[i, 1, 2], 1.0]))
        n = np.array([np.sin(tilt[i]) * np.cos(phi[i]), np.sin(tilt[i]) * np.sin(phi[i]), np.cos(tilt[i])])
        H = K @ (ROT + np.outer(TRANS, n) / (n @ X)) @ Ki
        l2[i] = sp.reproject_lafs(l1[i:i + 1], H)[0]
    l2[:, :, 2] += rng.normal(0.0, 0.3, (T, 2))
    l2[:, :, :2] *= 1.0 + 0.03 * rng.normal(0.0, 1.0, (T, 2, 2))
    out = rng.uniform(0, 1, T) < outlier_share
    fresh = sp.random_frames(rng, T)
    l2[out] = fresh[out]
    perm = rng.permutation(T)
    l2s = np.empty_like(l2)
    l2s[perm] = l2                       # frame t of image 2 lives in row perm[t]
    tent = np.stack([np.arange(T), perm], 1).astype(np.int32)
    return l1.astype(np.float32), l2s.astype(np.float32), tent, ~out, planted_F()


def few_rows():
    """Five consistent rows and nothing else: every hypothesis has at most 5 inliers, too few for a refit (flag 2)."""
    l1, l2, tent, _, _ = planted_two_view(40, 0.0, 21)
    return l1, l2, tent[:5]


def collinear_rows():
    """A depth scene whose image-1 centres all lie on the line y = 300 (exactly, also in float32): the hypotheses, which use the frames' tips
    too, are valid, but the normal matrix of the masked CENTRES has three exact null vectors (flag 4)."""
    fr = sp.random_frames(np.random.default_rng(23), 40)
    fr[:, 1, 2] = 300.0
    l1, l2, tent, _, _ = planted_two_view(40, 0.0, 24, frames1=fr)
    return l1, l2, tent


# ---- hash and members ------------------------------------------------------------------------------------------------------------------
_M = np.uint64(0xFFFFFFFF)


def lowbias32(x):
    x = np.asarray(x, np.uint64) & _M
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M
    return x ^ (x >> np.uint64(16))


def members(T, rounds, seed):
    """-> (T * rounds, 3) int64, row h = s * rounds + r; T >= 3."""
    assert T >= 3
    s = np.repeat(np.arange(T, dtype=np.uint64), rounds)
    r = np.tile(np.arange(rounds, dtype=np.uint64), T)
    m = [s.astype(np.int64)]
    for k in (1, 2):
        x = ((s * np.uint64(0x9E3779B1)) & _M) ^ ((r * np.uint64(0x85EBCA77)) & _M) ^ np.uint64((k * 0xC2B2AE3D) & 0xFFFFFFFF) ^ np.uint64(seed & 0xFFFFFFFF)
        j = ((lowbias32(x) * np.uint64(T)) >> np.uint64(32)).astype(np.int64)
        while True:
            dup = j == m[0]
            if k == 2:
                dup |= j == m[1]
            if not dup.any():
                break
            j = np.where(dup, (j + 1) % T, j)
        m.append(j)
    return np.stack(m, 1)


# ---- prep ------------------------------------------------------------------------------------------------------------------------------
def gather(lafs1, lafs2, tent):
    """-> pts (T,4) f64 centres (NaN rows for matches that are not usable), frm (T,12) f64 [a b x c d y | a2 b2 x2 c2 d2 y2] (NaN rows for
    matches that are not usable as members), match_ok, member_ok."""
    lafs1, lafs2, tent = np.asarray(lafs1, np.float32), np.asarray(lafs2, np.float32), np.asarray(tent).reshape(-1, 2)
    T = tent.shape[0]
    i, j = tent[:, 0].astype(np.int64), tent[:, 1].astype(np.int64)
    inr = (i >= 0) & (i < len(lafs1)) & (j >= 0) & (j < len(lafs2))
    frm = np.full((T, 12), np.nan)
    frm[inr] = np.concatenate([lafs1[i[inr]].reshape(-1, 6), lafs2[j[inr]].reshape(-1, 6)], 1).astype(np.float64)
    pts = frm[:, [2, 5, 8, 11]].copy()
    match_ok = inr & np.isfinite(pts).all(1)
    member_ok = inr & np.isfinite(frm).all(1)
    pts[~match_ok] = np.nan
    frm[~member_ok] = np.nan
    return pts, frm, match_ok, member_ok


# ---- solve -----------------------------------------------------------------------------------------------------------------------------
def denormalise(F, s1, cx1, cy1, s2, cx2, cy2):
    """F (H,9) normalised -> (F (H,9) of unit norm with the sign rule, ok (H,))."""
    F = np.asarray(F, np.float64)
    tx1, ty1, tx2, ty2 = -s1 * cx1, -s1 * cy1, -s2 * cx2, -s2 * cy2
    G = np.empty_like(F)
    for r in range(3):
        G[:, 3 * r] = F[:, 3 * r] * s1
        G[:, 3 * r + 1] = F[:, 3 * r + 1] * s1
        G[:, 3 * r + 2] = (F[:, 3 * r] * tx1 + F[:, 3 * r + 1] * ty1) + F[:, 3 * r + 2]
    O = np.empty_like(F)
    for c in range(3):
        O[:, c] = s2 * G[:, c]
        O[:, 3 + c] = s2 * G[:, 3 + c]
        O[:, 6 + c] = (tx2 * G[:, c] + ty2 * G[:, 3 + c]) + G[:, 6 + c]
    n2 = np.zeros(len(F))
    for i in range(9):
        n2 = n2 + O[:, i] * O[:, i]
    n = np.sqrt(n2)
    ok = (n > 0) & np.isfinite(n)
    O = O / n[:, None]
    a = np.where(np.isnan(O), -1.0, np.abs(O))
    big = np.argmax(a, 1)                                    # the first of the largest
    sign = np.where(O[np.arange(len(O)), big] < 0, -1.0, 1.0)
    return sign[:, None] * O, ok


def solve(frm, mem):
    """The 8-point solve of every hypothesis -> F (H,9) float64 (NaN rows for invalid hypotheses), ok (H,)."""
    H = len(mem)
    ar = np.arange(H)
    with np.errstate(all="ignore"):
        f = frm[mem]                                          # (H,3,12)
        ok = np.isfinite(f).all((1, 2))
        a, b, x, c, d, y = (f[:, :, k] for k in range(6))
        a2, b2, x2, c2, d2, y2 = (f[:, :, k] for k in range(6, 12))
        X = np.stack([x, x + a, x + b], 2).reshape(H, 9)
        Y = np.stack([y, y + c, y + d], 2).reshape(H, 9)
        U = np.stack([x2, x2 + a2, x2 + b2], 2).reshape(H, 9)
        V = np.stack([y2, y2 + c2, y2 + d2], 2).reshape(H, 9)
        cen = []
        for P in (X, Y, U, V):
            s = np.zeros(H)
            for p in range(9):
                s = s + P[:, p]
            cen.append(s / 9.0)
        cx1, cy1, cx2, cy2 = cen
        md1, md2 = np.zeros(H), np.zeros(H)
        for p in range(9):
            ax, ay, bx, by = X[:, p] - cx1, Y[:, p] - cy1, U[:, p] - cx2, V[:, p] - cy2
            md1 = md1 + np.sqrt(ax * ax + ay * ay)
            md2 = md2 + np.sqrt(bx * bx + by * by)
        md1, md2 = md1 / 9.0, md2 / 9.0
        s1, s2 = 1.4142135623730951 / md1, 1.4142135623730951 / md2
        ok &= (s1 > 0) & (s2 > 0) & np.isfinite(s1) & np.isfinite(s2)
        A = np.empty((H, 8, 9))
        for p in range(8):
            xn, yn, un, vn = (X[:, p] - cx1) * s1, (Y[:, p] - cy1) * s1, (U[:, p] - cx2) * s2, (V[:, p] - cy2) * s2
            A[:, p] = np.stack([un * xn, un * yn, un, vn * xn, vn * yn, vn, xn, yn, np.ones(H)], 1)
        perm = np.tile(np.arange(9), (H, 1))
        for k in range(8):
            sub = np.abs(A[:, k:8, k:9]).reshape(H, -1)
            sub = np.where(np.isnan(sub), -1.0, sub)
            idx = np.argmax(sub, 1)                           # row-major first maximum: smallest row, then smallest column
            ok &= sub[ar, idx] >= 1e-12
            pr, pc = k + idx // (9 - k), k + idx % (9 - k)
            row = A[ar, k, :].copy(); A[ar, k, :] = A[ar, pr, :]; A[ar, pr, :] = row
            col = A[ar, :, k].copy(); A[ar, :, k] = A[ar, :, pc]; A[ar, :, pc] = col
            pk = perm[ar, k].copy(); perm[ar, k] = perm[ar, pc]; perm[ar, pc] = pk
            fac = A[:, k + 1:8, k] / A[:, k, k][:, None]
            A[:, k + 1:8, k + 1:9] = A[:, k + 1:8, k + 1:9] - fac[:, :, None] * A[:, k, None, k + 1:9]
        yv = np.ones((H, 9))
        for i in range(7, -1, -1):
            s = A[:, i, 8].copy()
            for j in range(i + 1, 8):
                s = s + A[:, i, j] * yv[:, j]
            yv[:, i] = -s / A[:, i, i]
        Fn = np.empty((H, 9))
        for j in range(9):
            Fn[ar, perm[:, j]] = yv[:, j]
        F, fin = denormalise(Fn, s1, cx1, cy1, s2, cx2, cy2)
        ok &= fin
    F[~ok] = np.nan
    return F, ok


# ---- score -----------------------------------------------------------------------------------------------------------------------------
def _tree(F, pts, dtype):
    """e (H,T) by the header's expression tree in `dtype`, no fused multiply-add."""
    F = np.asarray(F, dtype).reshape(-1, 9)[:, None, :]
    p = np.asarray(pts, dtype)
    x, y, u, v = p[None, :, 0], p[None, :, 1], p[None, :, 2], p[None, :, 3]
    with np.errstate(all="ignore"):
        l0 = (F[..., 0] * x + F[..., 1] * y) + F[..., 2]
        l1 = (F[..., 3] * x + F[..., 4] * y) + F[..., 5]
        l2 = (F[..., 6] * x + F[..., 7] * y) + F[..., 8]
        m0 = (F[..., 0] * u + F[..., 3] * v) + F[..., 6]
        m1 = (F[..., 1] * u + F[..., 4] * v) + F[..., 7]
        r = (u * l0 + v * l1) + l2
        return (r * r) / (((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1)


def score_fp32(hyp32, pts, th):
    """The device's fp32 scoring of float32 models (H,9) -> counts (H,), inl (H,T), sqrt(e) as float64."""
    e = _tree(hyp32, pts, np.float32)
    with np.errstate(all="ignore"):
        inl = e <= np.float32(th) * np.float32(th)           # NaN, x/0 -> False
        return inl.sum(1).astype(np.int64), inl, np.sqrt(e.astype(np.float64))


def sampson(F, pts):
    """sqrt of the Sampson error in float64, (H,T) (or (T,) for one model); NaN for matches that are not usable."""
    F = np.asarray(F, np.float64)
    with np.errstate(all="ignore"):
        e = np.sqrt(_tree(F, pts, np.float64))
    return e[0] if F.size == 9 else e


# ---- local optimisation ----------------------------------------------------------------------------------------------------------------
def jacobi(A):
    """Cyclic Jacobi, exactly SWEEPS sweeps -> (diagonal, V with the eigenvectors as columns)."""
    A = np.array(A, np.float64)
    n = len(A)
    V = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[p, q]
                    if apq == 0.0:
                        continue
                    theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                    t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    xp, xq = A[:, p].copy(), A[:, q].copy()
                    A[:, p], A[:, q] = c * xp - s * xq, s * xp + c * xq
                    xp, xq = A[p, :].copy(), A[q, :].copy()
                    A[p, :], A[q, :] = c * xp - s * xq, s * xp + c * xq
                    xp, xq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * xp - s * xq, s * xp + c * xq
    return np.diag(A).copy(), V


def fit(p1, p2):
    """Rank-2 least-squares F of the pairs p1 <-> p2 (n >= 8) by the header's refit; None when degenerate."""
    n = len(p1)
    with np.errstate(all="ignore"):
        c1, c2 = p1.sum(0) / n, p2.sum(0) / n
        m1, m2 = np.sqrt(((p1 - c1) ** 2).sum(1)).sum() / n, np.sqrt(((p2 - c2) ** 2).sum(1)).sum() / n
        s1, s2 = 1.4142135623730951 / m1, 1.4142135623730951 / m2
        if not (s1 > 0 and s2 > 0 and np.isfinite(s1) and np.isfinite(s2)):
            return None
        q1, q2 = (p1 - c1) * s1, (p2 - c2) * s2
        x, y, u, v = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
        R = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones(n)], 1)
        w, V = jacobi(R.T @ R)
        if not np.isfinite(w).all():
            return None
        e = int(np.argmin(w))
        if not (np.delete(w, e).min() > 1e-12 * w.max()):
            return None
        Fn = V[:, e].reshape(3, 3)
        M = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                M[i, j] = (Fn[0, i] * Fn[0, j] + Fn[1, i] * Fn[1, j]) + Fn[2, i] * Fn[2, j]
        w3, V3 = jacobi(M)
        if not np.isfinite(w3).all():
            return None
        vv = V3[:, int(np.argmin(w3))]
        Fn = Fn - np.outer(Fn @ vv, vv)
        F, ok = denormalise(Fn.reshape(1, 9), s1, c1[0], c1[1], s2, c2[0], c2[1])
    return F[0] if ok[0] else None


def refine(pts, model0, start_mask, th, lo_iters, best, best_count=None):
    """The local optimisation from model 0 (9,) and its start mask.
    -> dict: F (9,), mask, summary, margin (smallest |sqrt(e) - th| over all matches and refit iterations; inf when none ran), near (T,) bool:
    matches within BAND of th under model 0 or in some iteration."""
    T = len(pts)
    if best < 0:
        return {"F": np.zeros(9), "mask": np.zeros(T, bool), "summary": [-1, 0, 0, 1], "margin": np.inf, "near": np.zeros(T, bool)}
    cur = np.asarray(start_mask, bool).copy()
    keep_F, keep_mask, flags, margin = np.asarray(model0, np.float64).reshape(9), cur.copy(), 0, np.inf
    with np.errstate(all="ignore"):
        near = np.abs(sampson(keep_F, pts) - th) <= BAND
    for _ in range(lo_iters):
        if cur.sum() < 8:
            flags |= 2
            break
        F = fit(pts[cur, 0:2], pts[cur, 2:4])
        if F is None:
            flags |= 4
            break
        err = sampson(F, pts)
        with np.errstate(all="ignore"):
            cur = err <= th
            near |= np.abs(err - th) <= BAND
            margin = min(margin, float(np.nanmin(np.abs(err - th))))
        if cur.sum() > keep_mask.sum():
            keep_F, keep_mask = F, cur.copy()
    bc = int(np.asarray(start_mask).sum()) if best_count is None else int(best_count)
    return {"F": keep_F, "mask": keep_mask, "summary": [int(best), bc, int(keep_mask.sum()), flags], "margin": margin, "near": near}


def hypotheses(lafs1, lafs2, tent, rounds, seed):
    """-> dict: pts, frm, match_ok, member_ok, mem (H,3) or None, F (H,9) float64, hyp32 (H,9) float32 (what the device stores), ok (H,)."""
    pts, frm, match_ok, member_ok = gather(lafs1, lafs2, tent)
    T = len(pts)
    if T < 3:
        F, ok, mem = np.full((T * rounds, 9), np.nan), np.zeros(T * rounds, bool), None
    else:
        mem = members(T, rounds, seed)
        F, ok = solve(frm, mem)
    return {"pts": pts, "frm": frm, "match_ok": match_ok, "member_ok": member_ok, "mem": mem, "F": F, "hyp32": F.astype(np.float32), "ok": ok}


def verify(lafs1, lafs2, tent, th=2.0, rounds=8, seed=0, lo_iters=3):
    """All of it: hypotheses in float64 rounded to float32, the fp32 scoring, select, the float64 refit from the fp32 inlier set."""
    hy = hypotheses(lafs1, lafs2, tent, rounds, seed)
    counts, inl, e32 = score_fp32(hy["hyp32"], hy["pts"], th)
    best = sp.select(counts)
    out = refine(hy["pts"], hy["hyp32"][best].astype(np.float64) if best >= 0 else None, inl[best] if best >= 0 else None, th, lo_iters, best,
                 counts[best] if best >= 0 else 0)
    out.update(counts=counts, best=best, inl=inl, e32=e32, hyp=hy)
    return out
