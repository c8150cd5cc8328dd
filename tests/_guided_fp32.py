"""numpy restatement of guided matching (include/affnet_hip.h: affnet_match_guided, affnet_guided_mask; affnet_amd/csrc/guided.hip), operation
by operation in float32, and the scenes its tests run on.  numpy and the other restatements only: no torch, no affnet_amd, no GPU.

  distance    _match_fp32.distance: the element affnet_distance_matrix writes
  planar      m = float32(model); X = (m0 x + m1 y) + m2, Y, W alike; px = X / W, py = Y / W; W > 0 && (dx dx + dy dy) <= r r
  epipolar    _epipolar_fp64._tree in float32 on the same float32 model; e <= r r
  order       a NaN distance first, then the smaller distance, then the smaller index - first_k, used for rows and (transposed) for columns
  selection   idx0 >= 0 && d0 <= max_dist && d0 / (d1 + 1e-8f) <= thr [&& back[idx0] == row], kept pairs in row order

tests/test_guided_host.py pins these functions and proves that the scenes contain what they claim; tests/test_gpu_guided.py compares the
kernels with them on the bytes."""
import numpy as np

import _epipolar_fp64 as ep
import _match_fp32 as mf
import _spatial_fp64 as sp

F32 = np.float32
PLANAR, EPIPOLAR = 0, 1
# px: ten times the largest |sqrt(e32) - sqrt(e64)| of the planar transfer error over all pairs with sqrt(e64) < 2 r, MEASURED between
# planar_error(.., float32) and planar_error(.., float64) on the CPU over repeated_scene(T, T), T = 65, 130, 257 (r = 10, PLANTED_H) and
# dense_scene(65, 200) and (200, 415) (r = 40, DENSE_H): the largest was 8.88e-5 px; ten times that, rounded up to two
# digits.  test_band_is_ten_times_the_fp32_spread measures it again.
PLANAR_BAND = 8.9e-4
DENSE_H = np.array([[1.0, 0.02, 3.0], [-0.01, 1.0, -2.0], [1e-5, 2e-5, 1.0]])
DENSE_R = 40.0
NEG_W = np.diag([1.0, 1.0, -1.0])


# ---- the admissible test ---------------------------------------------------------------------------------------------------------------
def centres(lafs):
    lafs = np.asarray(lafs, F32)
    return lafs[:, 0, 2], lafs[:, 1, 2]


def planar_error(lafs1, lafs2, model, dtype=F32):
    """-> (e (n1,n2) squared transfer error, W (n1,)) by the header's tree in `dtype`, no fused multiply-add."""
    m = np.asarray(model, np.float64).reshape(9).astype(F32).astype(dtype)           # the device reads (float)model[k]
    x, y = (c.astype(dtype) for c in centres(lafs1))
    u, v = (c.astype(dtype) for c in centres(lafs2))
    with np.errstate(all="ignore"):
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        W = (m[6] * x + m[7] * y) + m[8]
        px, py = X / W, Y / W
        dx, dy = px[:, None] - u[None, :], py[:, None] - v[None, :]
        e = dx * dx + dy * dy
    assert e.dtype == dtype and W.dtype == dtype
    return e, W


def epipolar_error(lafs1, lafs2, model, dtype=F32):
    """-> e (n1,n2): the Sampson error of every pair by _epipolar_fp64._tree in `dtype`."""
    x, y = centres(lafs1)
    u, v = centres(lafs2)
    n1, n2 = len(x), len(u)
    pts = np.stack([np.repeat(x, n2), np.repeat(y, n2), np.tile(u, n1), np.tile(v, n1)], 1)
    F = np.asarray(model, np.float64).reshape(9).astype(F32)
    return ep._tree(F, pts, dtype)[0].reshape(n1, n2)


def admissible(lafs1, lafs2, model, kind, r):
    """affnet_guided_mask: (n1,n2) bool."""
    r2 = F32(r) * F32(r)
    with np.errstate(all="ignore"):
        if kind == PLANAR:
            e, W = planar_error(lafs1, lafs2, model)
            return (W > 0)[:, None] & (e <= r2)
        return epipolar_error(lafs1, lafs2, model) <= r2


# ---- order, lists, selection -----------------------------------------------------------------------------------------------------------
def first_k(M, adm, k):
    """Per row of M the first k columns with adm in the order (NaN, value, column) -> dist (n,k) float32, idx (n,k) int32; unfilled (+inf, -1)."""
    M, adm = np.asarray(M, F32), np.asarray(adm, bool)
    n = M.shape[0]
    dist, idx = np.full((n, k), np.inf, F32), np.full((n, k), -1, np.int32)
    for i in range(n):
        c = np.nonzero(adm[i])[0]
        v = M[i, c]
        nan = np.isnan(v)
        o = np.lexsort((c, np.where(nan, F32(0), v), ~nan))[:k]              # the last key is the first criterion
        dist[i, :len(o)], idx[i, :len(o)] = v[o], c[o]
    return dist, idx


def guided_from(M, adm, thr, max_dist=np.inf, mutual=True, closed=False):
    """affnet_match_guided from the distance matrix and the admissible matrix on -> dict(dist, idx, back, keep, tent (count,2) int32, count).
    closed: the gate says "no model"."""
    adm = np.asarray(adm, bool) & (not closed)
    dist, idx = first_k(M, adm, 2)
    back = first_k(np.asarray(M, F32).T, adm.T, 1)[1][:, 0]
    with np.errstate(all="ignore"):
        ratio = dist[:, 0] / (dist[:, 1] + mf.EPS_R)
        assert ratio.dtype == F32
        keep = (idx[:, 0] >= 0) & (dist[:, 0] <= F32(max_dist)) & (ratio <= F32(thr))
    if mutual:
        keep &= back[np.maximum(idx[:, 0], 0)] == np.arange(len(idx))
    rows = np.nonzero(keep)[0]
    tent = np.stack([rows, idx[rows, 0]], 1).astype(np.int32).reshape(-1, 2)
    return dict(dist=dist, idx=idx, back=back.astype(np.int32), keep=keep, tent=tent, count=int(rows.size), adm=adm)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


_SCENES = {}


def repeated_scene(T, seed, kind=PLANAR):
    """Repeated structure: dict(d1 (T,128), d2 (n2,128), l1 (T,2,3), l2 (n2,2,3), model (3,3) float64, partner (T,) int (-1: not planted),
    repeated (T,) bool, decoy (T,) int), made once and never modified.
    Frames: _spatial_fp64.planted(T, seed) with PLANTED_H (planar) or _epipolar_fp64.planted_two_view(T, 0.5, seed) with its F (epipolar).
    Descriptors: every planted row and its partner are noisy unit copies (0.03 per component) of one pool row, everything else is random.  A
    third of the planted rows are `repeated`: image 2 gets one more row, decoy[i], with another noisy copy of the same pool row, on a random
    frame more than 100 px from where H sends the row's centre (planar) or more than 50 px, by float64 Sampson distance, from its epipolar
    line (epipolar)."""
    key = (T, seed, kind)
    if key in _SCENES:
        return _SCENES[key]
    if kind == PLANAR:
        l1, l2, tent, pl = sp.planted(T, seed)
        model = sp.PLANTED_H.copy()
    else:
        l1, l2, tent, pl, model = ep.planted_two_view(T, 0.5, seed)
    rng = np.random.default_rng(7919 * T + seed + 31 * kind)
    rows = np.nonzero(pl)[0]
    rep_rows = rows[::3]
    pool = _unit(rng.normal(size=(T, 128)))
    d1 = _unit(rng.normal(size=(T, 128)))
    d2 = _unit(rng.normal(size=(T + len(rep_rows), 128)))
    d1[rows] = _unit(pool[rows] + 0.03 * rng.normal(size=(len(rows), 128)))
    d2[tent[rows, 1]] = _unit(pool[rows] + 0.03 * rng.normal(size=(len(rows), 128)))
    d2[T:] = _unit(pool[rep_rows] + 0.03 * rng.normal(size=(len(rep_rows), 128)))
    extra = np.empty((len(rep_rows), 2, 3))
    for k, i in enumerate(rep_rows):
        while True:
            fr = sp.random_frames(rng, 1)
            pts = np.array([[l1[i, 0, 2], l1[i, 1, 2], fr[0, 0, 2], fr[0, 1, 2]]], np.float64)
            far = sp.transfer(model, pts)[0][0] > 100.0 if kind == PLANAR else ep.sampson(model.reshape(9), pts)[0] > 50.0
            if far:
                break
        extra[k] = fr[0]
    partner = np.full(T, -1, np.int64)
    partner[rows] = tent[rows, 1]
    repeated, decoy = np.zeros(T, bool), np.full(T, -1, np.int64)
    repeated[rep_rows], decoy[rep_rows] = True, T + np.arange(len(rep_rows))
    out = dict(d1=d1.astype(F32), d2=d2.astype(F32), l1=l1, l2=np.concatenate([l2, extra.astype(F32)]), model=np.asarray(model, np.float64).reshape(3, 3),
               partner=partner, repeated=repeated, decoy=decoy)
    for v in out.values():
        v.setflags(write=False)
    _SCENES[key] = out
    return out


def dense_scene(n1, n2):
    """Many admissible columns per row: dict(d1, d2, l1, l2, model = DENSE_H (planar; radius DENSE_R = 40)), made once and never modified.
    The descriptors are _match_fp32.planted(n1, n2): duplicate columns in the same and in another tile lane, NaN self-distances, exact copies.
    The centres of image 2 are uniform in a 120 x 120 px window and DENSE_H sends the centres of image 1 to uniform places in it.  For
    n1 >= 23 and n2 >= 40 also: row 0 (a copy of column 5 = column 21) lands next to columns 5 and 21, row n1 - 2 (a copy of column 0, NaN
    distance) next to column 0, row 1 lands in the corner (0, 0), which no column comes near, and row 2 in the corner (120, 0), where column 3
    is alone."""
    key = ("dense", n1, n2)
    if key in _SCENES:
        return _SCENES[key]
    d1, d2 = mf.planted(n1, n2)
    rng = np.random.default_rng(15485863 + 1009 * n1 + n2)
    c2 = rng.uniform(0.0, 120.0, (n2, 2))
    t1 = rng.uniform(0.0, 120.0, (n1, 2))
    if n1 >= 23 and n2 >= 40:
        reach = DENSE_R + 5.0
        for corner in (np.array([0.0, 0.0]), np.array([120.0, 0.0])):
            near = np.sqrt(((c2 - corner) ** 2).sum(1)) < reach
            c2[near] = 120.0 - c2[near]                                                    # through the centre, to the opposite corner
        c2[3] = (112.0, 9.0)
        c2[5], c2[21] = (60.0, 60.0), (66.0, 63.0)
        c2[0] = (30.0, 90.0)
        t1[0], t1[1], t1[2], t1[n1 - 2] = (62.0, 61.0), (0.0, 0.0), (120.0, 0.0), (31.0, 91.0)
    Hi = np.linalg.inv(DENSE_H)
    p = np.concatenate([t1, np.ones((n1, 1))], 1) @ Hi.T
    c1 = p[:, :2] / p[:, 2:3]

    def frames(c):
        f = np.zeros((len(c), 2, 3))
        f[:, 0, 0] = f[:, 1, 1] = 10.0
        f[:, :, 2] = c
        return f.astype(F32)
    out = dict(d1=d1, d2=d2, l1=frames(c1), l2=frames(c2), model=DENSE_H.copy())
    for v in out.values():
        v.setflags(write=False)
    _SCENES[key] = out
    return out


_DIST = {}


def scene_distance(name, sc):
    """_match_fp32.distance of a scene's descriptors, computed once per scene."""
    if name not in _DIST:
        _DIST[name] = mf.distance(sc["d1"], sc["d2"])
    return _DIST[name]


def boundary_pairs():
    """Integer centres for r = 5 under the identity and under NEG_W: l1 (5,2,3), l2 (3,2,3).
    rows: 0 at (10, 20); 1 at (-10, -20), which NEG_W = diag(1, 1, -1) sends onto column 2 with W = -1; 2, 3 with a NaN centre; 4 far away
    columns: 0 at (13, 24): offset (3, 4) from row 0, 25 <= 25; 1 at (nextafter(13), 24): one ulp too far; 2 at (10, 20)"""
    def frames(c):
        f = np.zeros((len(c), 2, 3), F32)
        f[:, 0, 0] = f[:, 1, 1] = 5.0
        f[:, :, 2] = np.asarray(c, F32)
        return f
    l1 = frames([(10, 20), (-10, -20), (np.nan, 20), (10, np.nan), (500, 500)])
    l2 = frames([(13, 24), (np.nextafter(F32(13), F32(14)), 24), (10, 20)])
    return l1, l2
