"""numpy restatement of ratio-test matching (include/affnet_hip.h: affnet_match_ratio; affnet_amd/csrc/ratio_match.hip), operation by operation
in float32, and the scenes its tests run on.  numpy and the other restatements only: no torch, no affnet_amd, no GPU.

  distance      _match_fp32.distance: the element affnet_distance_matrix writes
  order         a NaN distance first, then the smaller distance, then the smaller index (_guided_fp32.first_k)
  slot 0        the first column of the row over all columns
  inconsistent  radius < 0: every column; else du = u[j] - u[j1], dv = v[j] - v[j1]; !((du du + dv dv) <= r r), one rounding per operation
  slot 1        the first column j != idx0 that is inconsistent with idx0; unfilled (+inf, -1)
  back          the first row of every column, no geometry
  selection     idx0 >= 0 && d0 <= max_dist && d0 / (d1 + 1e-8f) <= thr [&& back[idx0] == row], kept pairs in row order

tests/test_ratio_mirror_host.py pins these functions and proves that the scenes contain what they claim; tests/test_gpu_ratio_match.py compares
the kernels with them on the bytes."""
import numpy as np

import _guided_fp32 as gf
import _match_fp32 as mf

F32 = np.float32


def inconsistent(l2, idx0, radius):
    """(n1, n2) bool: column j against the centre of column idx0[i], for every row i.  radius < 0: all true."""
    u, v = gf.centres(l2) if l2 is not None else (np.zeros(0, F32), np.zeros(0, F32))
    n1 = len(idx0)
    if radius < 0:
        return np.ones((n1, 0 if l2 is None else len(u)), bool)
    if len(u) == 0:
        return np.ones((n1, 0), bool)
    j1 = np.maximum(np.asarray(idx0), 0)
    with np.errstate(all="ignore"):
        r2 = F32(radius) * F32(radius)
        du, dv = u[None, :] - u[j1][:, None], v[None, :] - v[j1][:, None]
        e = du * du + dv * dv
        assert e.dtype == F32 and r2.dtype == F32
        return ~(e <= r2)


def ratio_from(M, l2, radius, thr, max_dist=np.inf, mutual=False):
    """affnet_match_ratio from the distance matrix on -> dict(dist (n1,2), idx (n1,2), back, ratio, keep, tent (count,2) int32, count)."""
    M = np.asarray(M, F32)
    n1, n2 = M.shape
    every = np.ones((n1, n2), bool)
    d0, i0 = gf.first_k(M, every, 1)
    inc = inconsistent(l2, i0[:, 0], radius) if radius >= 0 else every
    adm = inc & (np.arange(n2)[None, :] != i0[:, :1])
    d1, i1 = gf.first_k(M, adm, 1)
    dist, idx = np.concatenate([d0, d1], 1), np.concatenate([i0, i1], 1)
    back = gf.first_k(M.T, every.T, 1)[1][:, 0]
    with np.errstate(all="ignore"):
        ratio = dist[:, 0] / (dist[:, 1] + mf.EPS_R)
        assert ratio.dtype == F32
        keep = (idx[:, 0] >= 0) & (dist[:, 0] <= F32(max_dist)) & (ratio <= F32(thr))
    if mutual and n2:
        keep &= back[np.maximum(idx[:, 0], 0)] == np.arange(n1)
    rows = np.nonzero(keep)[0]
    tent = np.stack([rows, idx[rows, 0]], 1).astype(np.int32).reshape(-1, 2)
    return dict(dist=dist, idx=idx, back=back.astype(np.int32), ratio=ratio, keep=keep, tent=tent, count=int(rows.size))


def ratio_loops(M, l2, radius):
    """The two slots by a plain double loop over the candidates, scalar float32 arithmetic -> dist (n1,2), idx (n1,2)."""
    M = np.asarray(M, F32)
    n1, n2 = M.shape

    def before(d, c, s, sc):          # topk.h, topk_before
        dn, sn = np.isnan(d), np.isnan(s)
        if dn:
            return (not sn) or c < sc
        return (not sn) and (d < s or (d == s and c < sc))
    dist, idx = np.full((n1, 2), np.inf, F32), np.full((n1, 2), -1, np.int32)
    if n2 == 0:
        return dist, idx
    u, v = gf.centres(l2) if radius >= 0 else (None, None)
    with np.errstate(all="ignore"):
        r2 = F32(radius) * F32(radius)
    for i in range(n1):
        b = 0
        for j in range(1, n2):
            if before(M[i, j], j, M[i, b], b):
                b = j
        dist[i, 0], idx[i, 0] = M[i, b], b
        s = -1
        for j in range(n2):
            if j == b:
                continue
            if radius >= 0:
                with np.errstate(all="ignore"):
                    du, dv = F32(u[j] - u[b]), F32(v[j] - v[b])
                    if F32(F32(du * du) + F32(dv * dv)) <= r2:
                        continue
            if s < 0 or before(M[i, j], j, M[i, s], s):
                s = j
        if s >= 0:
            dist[i, 1], idx[i, 1] = M[i, s], s
    return dist, idx


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def frames(c):
    f = np.zeros((len(c), 2, 3), F32)
    f[:, 0, 0] = f[:, 1, 1] = 8.0
    f[:, :, 2] = np.asarray(c, F32).reshape(-1, 2)
    return f


_CACHE = {}


def _frozen(key, make):
    if key not in _CACHE:
        out = make()
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def planted_scene(n1, n2):
    """_match_fp32.planted(n1, n2) with centres for image 2: uniform in a 60 x 60 px window (a radius of 10 px holds about one column in
    twelve), and every third column on exactly the place of the column before it.  For n2 >= 40 the duplicate descriptors of that input
    (_match_fp32.DUP_SAME_LANE, DUP_OTHER_LANE) also share places: column 21 lies exactly on column 5 (radius 0 makes a difference for the
    rows that copy them) and column 38 at offset (3, 4) from column 7 (radius 10 does, radius 0 does not).  dict(d1, d2, l2)."""
    def make():
        d1, d2 = mf.planted(n1, n2)
        c = np.random.default_rng(32452843 + 1013 * n1 + n2).uniform(0.0, 60.0, (n2, 2))
        c[2::3] = c[1::3][:len(c[2::3])]
        if n2 >= 40:
            c[21] = c[5]
            c[38] = c[7] + (3.0, 4.0)
        return dict(d1=d1, d2=d2, l2=frames(c))
    return _frozen(("planted", n1, n2), make)


_M = {}


def scene_distance(key, sc):
    """_match_fp32.distance of a scene's descriptors, computed once per scene."""
    if key not in _M:
        _M[key] = mf.distance(sc["d1"], sc["d2"])
    return _M[key]


TWINS = 40


def twin_scene():
    """(a) n1 = 70, n2 = 130.  Rows 0 .. 39 are planted: column i is the partner (both 0.03 copies of one pool row) and column 40 + i its twin,
    1.5 px away, a 0.035 copy of the same pool row - the ratio of the two is about 0.92.  Rows 40 .. 69 and columns 80 .. 129 are random; the
    centres are uniform in 640 x 480.  dict(d1, d2, l2, planted (rows))."""
    def make():
        rng = np.random.default_rng(86028121)
        T = TWINS
        pool = _unit(rng.normal(size=(T, 128)))
        d1, d2 = _unit(rng.normal(size=(70, 128))), _unit(rng.normal(size=(130, 128)))
        d1[:T] = _unit(pool + 0.03 * rng.normal(size=(T, 128)))
        d2[:T] = _unit(pool + 0.03 * rng.normal(size=(T, 128)))
        d2[T:2 * T] = _unit(pool + 0.035 * rng.normal(size=(T, 128)))
        c = rng.uniform(0.0, 1.0, (130, 2)) * (640.0, 480.0)
        ang = rng.uniform(0.0, 2 * np.pi, T)
        c[T:2 * T] = c[:T] + 1.5 * np.stack([np.cos(ang), np.sin(ang)], 1)
        return dict(d1=d1.astype(F32), d2=d2.astype(F32), l2=frames(c), planted=np.arange(T))
    return _frozen("twin", make)


def nine_scene():
    """(b) n1 = 4, n2 = 60.  Row 0: columns 20 .. 29 are ten copies of its vector with noise 0.020 .. 0.029, all within 3 px of each other:
    whichever is the nearest, the other nine share its place; column 45, 200 px away, is the next one (noise 0.08).  A list of eight second
    candidates never sees column 45."""
    def make():
        rng = np.random.default_rng(49979687)
        d1, d2 = _unit(rng.normal(size=(4, 128))), _unit(rng.normal(size=(60, 128)))
        p = d1[0]
        for k in range(10):
            d2[20 + k] = _unit((p + (0.02 + 0.001 * k) * rng.normal(size=128))[None])[0]
        d2[45] = _unit((p + 0.08 * rng.normal(size=128))[None])[0]
        c = rng.uniform(300.0, 600.0, (60, 2))
        c[20:30] = (100.0, 100.0) + rng.uniform(-1.0, 1.0, (10, 2))
        c[45] = (300.0, 100.0)
        return dict(d1=d1.astype(F32), d2=d2.astype(F32), l2=frames(c))
    return _frozen("nine", make)


def boundary_scene():
    """(c) n1 = 1, n2 = 20, integer centres.  Column 0 at (100, 100) is the nearest; column 1 at (106, 108), offset (6, 8): 36 + 64 <= 100,
    consistent at radius 10; column 2 at (106, nextafter(108)): inconsistent.  Their descriptors are the second and third nearest."""
    def make():
        rng = np.random.default_rng(67867967)
        d1, d2 = _unit(rng.normal(size=(1, 128))), _unit(rng.normal(size=(20, 128)))
        for k, s in enumerate((0.01, 0.02, 0.03)):
            d2[k] = _unit((d1[0] + s * rng.normal(size=128))[None])[0]
        c = np.zeros((20, 2), F32)
        c[:] = rng.integers(300, 600, (20, 2))
        c[0], c[1] = (100, 100), (106, 108)
        c[2] = (106, np.nextafter(F32(108), F32(109)))
        return dict(d1=d1.astype(F32), d2=d2.astype(F32), l2=frames(c))
    return _frozen("boundary", make)


def duplicate_scene():
    """(d) n1 = 3, n2 = 40.  Row 0: columns 3 and 7 hold one vector, the nearest - slot 0 is column 3, slot 1 column 7 at the same distance
    (their centres are 200 px apart).  Row 1: column 9 is the nearest, columns 10 and 12 hold one vector, the second nearest - slot 1 is 10.
    Columns 19 and 35 (lane 3 of two tiles) hold one vector, the nearest of row 2."""
    def make():
        rng = np.random.default_rng(15487469)
        d1, d2 = _unit(rng.normal(size=(3, 128))), _unit(rng.normal(size=(40, 128)))
        d2[3] = _unit((d1[0] + 0.02 * rng.normal(size=128))[None])[0]
        d2[7] = d2[3]
        d2[9] = _unit((d1[1] + 0.02 * rng.normal(size=128))[None])[0]
        d2[10] = _unit((d1[1] + 0.05 * rng.normal(size=128))[None])[0]
        d2[12] = d2[10]
        d2[35] = _unit((d1[2] + 0.02 * rng.normal(size=128))[None])[0]
        d2[19] = d2[35]
        c = np.stack([np.arange(40) * 200.0, np.arange(40) * 50.0], 1)
        return dict(d1=d1.astype(F32), d2=d2.astype(F32), l2=frames(c))
    return _frozen("duplicate", make)


def crowded_scene():
    """(e) n1 = 2, n2 = 6: every column within 3 px of every other.  At radius 10 no column is inconsistent with any nearest one."""
    def make():
        rng = np.random.default_rng(32452867)
        d1, d2 = _unit(rng.normal(size=(2, 128))), _unit(rng.normal(size=(6, 128)))
        d2[4] = _unit((d1[0] + 0.02 * rng.normal(size=128))[None])[0]
        c = (50.0, 50.0) + rng.uniform(-1.0, 1.0, (6, 2))
        return dict(d1=d1.astype(F32), d2=d2.astype(F32), l2=frames(c))
    return _frozen("crowded", make)


def nan_scene():
    """(f) n1 = 3, n2 = 24.  Column 6 is a vector of length 16 whose distance to itself has a negative radicand in the kernels' arithmetic, row 1
    is that vector: its nearest distance is NaN.  Rows 0 and 2 are 0.03 copies of columns 2 and 11."""
    def make():
        rng = np.random.default_rng(49979693)
        d1, d2 = _unit(rng.normal(size=(3, 128))).astype(F32), _unit(rng.normal(size=(24, 128))).astype(F32)
        d1[0] = _unit((d2[2] + 0.03 * rng.normal(size=128))[None])[0]
        d1[2] = _unit((d2[11] + 0.03 * rng.normal(size=128))[None])[0]
        for _ in range(64):
            d2[6] = F32(16.0) * _unit(rng.normal(size=(1, 128)))[0].astype(F32)
            if np.isnan(mf.distance(d2[6:7], d2[6:7])[0, 0]):
                break
        d1[1] = d2[6]
        return dict(d1=d1, d2=d2, l2=frames(rng.uniform(0.0, 400.0, (24, 2))))
    return _frozen("nan", make)


def single_scene():
    """(g) n1 = 5, n2 = 1."""
    def make():
        rng = np.random.default_rng(86028157)
        return dict(d1=_unit(rng.normal(size=(5, 128))).astype(F32), d2=_unit(rng.normal(size=(1, 128))).astype(F32), l2=frames([(7.0, 9.0)]))
    return _frozen("single", make)


def nan_centre_scene():
    """(h) n1 = 2, n2 = 12, every centre within 3 px.  Row 0: its nearest, column 4, has a NaN centre - every other column is inconsistent with it.
    Row 1: its nearest, column 8, has a finite centre; column 5 (u NaN) and column 6 (v NaN) are inconsistent with it, the rest consistent;
    column 6 is nearer than column 5."""
    def make():
        rng = np.random.default_rng(67867979)
        d1, d2 = _unit(rng.normal(size=(2, 128))), _unit(rng.normal(size=(12, 128)))
        d2[4] = _unit((d1[0] + 0.02 * rng.normal(size=128))[None])[0]
        d2[8] = _unit((d1[1] + 0.02 * rng.normal(size=128))[None])[0]
        d2[6] = _unit((d1[1] + 0.06 * rng.normal(size=128))[None])[0]
        d2[5] = _unit((d1[1] + 0.09 * rng.normal(size=128))[None])[0]
        c = (50.0, 50.0) + rng.uniform(-1.0, 1.0, (12, 2))
        c[4] = (np.nan, np.nan)
        c[5, 0] = np.nan
        c[6, 1] = np.nan
        return dict(d1=d1.astype(F32), d2=d2.astype(F32), l2=frames(c))
    return _frozen("nan_centre", make)


SPECIAL = dict(twin=twin_scene, nine=nine_scene, boundary=boundary_scene, duplicate=duplicate_scene, crowded=crowded_scene, nan=nan_scene,
               single=single_scene, nan_centre=nan_centre_scene)
