"""Planted response pyramids AND planted affine maps for the OnePassSIR detector (host only: torch CPU + the oracle, no GPU import).

OnePassSIR has two slots on both sides: RespNet(level, sigma) and the dense AffNet(level 0 of an octave) -> (1,4,h,w)
(OnePassOracle(resp_fn=..., aff_fn=...), affnet_amd.OnePassSIR(RespNet=..., AffNet=...)).  With both planted on an all-zero image,
everything the detector does behind them is discrete: the per-level cut `0 < N < n_pos` with its radix select and tie rule, the
four-corner test of the x 3.0 frame, the global top-N and the plane / octave / image indexing of the maps.  This module builds such
inputs (reusing tests/_planted.py) and turns the oracle's per-level rows into what the detector must return for a budget N.

tests/test_planted_onepass_oracle.py proves on the oracle alone that every construction reaches the branch it is named after;
tests/test_gpu_planted_onepass.py runs them through the kernels.

Geometry used throughout (LAF.py:442-449, OnePassSIR.py:95): an isolated maximum at pixel (y, x) of pyramid level l has the normalised
frame [s A | ((x + 0.5) / w, (y + 0.5) / h)] with s = sigma_l / min(h, w), and it is dropped when a corner
(cx + 3 s (a11 px + a12 py), cy + 3 s (a21 px + a22 py)), px, py = +-1, leaves [0, 1].  The builders place points with that formula;
whether a frame really is inside is always read off the oracle.
"""
import collections

import numpy as np
import torch

import _planted as pl
import affnet_oracle as orc
import onepass_oracle as opo

MR, BORDER = 5.192, 15           # border = 15: every octave is at least 34 px, which the OnePassSIR context demands
Planted = collections.namedtuple("Planted", "case maps")        # case: _planted.Case; maps: [(1,4,h,w) fp32 per octave] = (a11, a12, a21, a22)

INSIDE_A = (0.25, -0.05, 0.0625, 0.1875)     # the map away from the planted pixels: a small frame that stays inside everywhere
OUT_LEFT = (2.0, 1.5, 0.0625, 0.1875)        # pushes the corner (-1, -1) of a frame in the left quarter of the image past x = 0


def plan_of(H, W, nlevels=3):
    return pl.plan_of(H, W, nlevels, border=BORDER)


def octave_shapes(H, W, n):
    shapes, (h, w) = [], (int(H), int(W))
    for _ in range(n):
        shapes.append((h, w))
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert len(set(shapes)) == len(shapes)
    return shapes


def planted_aff_fn(H, W, maps):
    """A fresh callable fn(level 0 of an octave (1,1,h,w)) -> a copy of maps[octave]; the octave is read off the shape (as planted_fn
    does), so nothing depends on the order of the calls.  The result lives on the CPU: both sides move it where they need it."""
    shapes = octave_shapes(H, W, len(maps))
    for s, m in zip(shapes, maps):
        assert tuple(m.shape) == (1, 4) + s and m.dtype == torch.float32 and float(m.abs().max()) <= 2.0, (s, tuple(m.shape))

    def fn(level0):
        return maps[shapes.index((int(level0.shape[2]), int(level0.shape[3])))].clone()
    return fn


def by_image_value(fns):
    """batch case: image b is the constant b, so is every pyramid level of it (the Gaussian taps sum to 1 up to rounding): the slot
    callables pick the plant of image round(mean)"""
    def fn(level, *a):
        return fns[int(round(float(level.float().mean())))](level, *a)
    return fn


def slots(p):
    """(resp_fn, aff_fn) of a planted case"""
    c = p.case
    return (pl.planted_fn(c.H, c.W, c.plant, plan_of(c.H, c.W, c.kw.get("nlevels", 3))[1]), planted_aff_fn(c.H, c.W, p.maps))


# ---- reference rows ------------------------------------------------------------------------------------------------------------------------
def run_oracle(p, N, value=0.0):
    """the unmodified OnePassOracle on the constant image `value` with both slots planted -> (oracle, LAFs px, responses)"""
    c = p.case
    rf, af = slots(p)
    ex = opo.OnePassOracle(mrSize=MR, border=BORDER, num_features=N, nlevels=c.kw.get("nlevels", 3), resp_fn=rf, aff_fn=af)
    L, r = ex(torch.full((1, 1, c.H, c.W), float(value)), do_ori=False)
    return ex, L, r


def level_rows(p, value=0.0):
    """The oracle's keep-all rows per (octave, level) BEFORE the boundary filter, concatenated in (octave, level, pixel) order:
    dict(ids (n,3) int64, resp (n,) fp32 - negative rows included, lafs (n,2,3) fp32 pixels - as OnePassSIR.forward scales them,
    norm (n,2,3) fp32 normalised frames as NMS3dAndComposeAAff returns them, inside (n,) bool = checkTouchBoundary of the x 3.0 frame)."""
    c = p.case
    ex, _, _ = run_oracle(p, -1, value)
    ids, resp, norm, inside = [], [], [], []
    for e in ex.level_rows:
        n = e["pix"].numel()
        ids.append(np.stack([np.full(n, e["octave"], np.int64), np.full(n, e["level"], np.int64), e["pix"].numpy().astype(np.int64)], axis=1))
        resp.append(e["resp"].numpy())
        norm.append(e["lafs"])
        inside.append(e["inside"].numpy().astype(bool))
    norm = torch.cat(norm)
    px = norm.clone()
    px[:, 0:2, 0:2] = MR * px[:, :, 0:2]                                    # OnePassSIR.py:146
    px = orc.denormalize_lafs(px, c.W, c.H)                                 # :153
    rows = {"ids": np.concatenate(ids), "resp": np.concatenate(resp).astype(np.float32), "lafs": px.numpy().copy(), "norm": norm.numpy().copy(),
            "inside": np.concatenate(inside)}
    assert np.all(np.diff(pl.order_key(rows["ids"])) > 0)
    return rows


def level_cut(rows, N):
    """bool mask: the rows the per-level cut keeps.  Per (octave, level) with 0 < N < n_pos (n_pos: responses > 0 of the level): the first N
    of the level under (response descending, pixel ascending) - HandCraftedModules.py:323-327 is a torch.topk, whose choice among equal
    values is unspecified: pixel order is this project's rule; otherwise every row of the level, negative ones included."""
    keep = np.ones(len(rows["resp"]), dtype=bool)
    grp = rows["ids"][:, 0] * 64 + rows["ids"][:, 1]
    for g in np.unique(grp):
        idx = np.nonzero(grp == g)[0]
        r = rows["resp"][idx]
        if 0 < N < int((r > 0).sum()):
            order = np.lexsort((rows["ids"][idx, 2], -r.astype(np.float64)))
            keep[idx[order[N:]]] = False
    return keep


def select_rows_onepass(rows, N):
    """What the detector must return for num_features = N given level_rows(): the per-level cut (level_cut), THEN the rows whose frame
    is not inside are dropped (a row below the cut never replaces one the filter drops), then the budget rule of _planted.select_rows:
    more than N rows left -> the first N under (response descending, (octave, level, pixel) ascending), in that order; otherwise all of
    them in (octave, level, pixel) order."""
    keep = level_cut(rows, N) & rows["inside"]
    return pl.select_rows({k: rows[k][keep] for k in ("ids", "resp", "lafs")}, N)


def cut_report(rows, N):
    """{(octave, level): dict(n_pos, T, ties, need)} of the levels that N cuts: `ties` rows share the threshold response T, `need` of them
    are inside the cut"""
    out = {}
    grp = rows["ids"][:, 0] * 64 + rows["ids"][:, 1]
    for g in np.unique(grp):
        r = rows["resp"][grp == g]
        n_pos = int((r > 0).sum())
        if 0 < N < n_pos:
            T = np.sort(r)[::-1][N - 1]
            out[(int(g) // 64, int(g) % 64)] = {"n_pos": n_pos, "T": float(T), "ties": int((r == T).sum()), "need": N - int((r > T).sum())}
    return out


# ---- builders ------------------------------------------------------------------------------------------------------------------------------
def base_maps(shapes, a=INSIDE_A):
    """Per octave a (1,4,h,w) map around `a`, every plane different at every pixel of a 17 x 17 neighbourhood and in every octave (steps
    of 2^-10, exact in fp32): a read at a wrong pixel, plane or octave changes the frame by far more than the bar of the GPU test."""
    maps = []
    for o, (h, w) in enumerate(shapes):
        yy = torch.arange(h, dtype=torch.float32).view(h, 1).expand(h, w)
        xx = torch.arange(w, dtype=torch.float32).view(1, w).expand(h, w)
        m = torch.stack([a[i] * (1.0 + 0.125 * o) + torch.remainder(yy * (3 + i) + xx * (5 + 2 * i) + o, 17.0) * 2.0 ** -10 for i in range(4)])
        maps.append(m.view(1, 4, h, w).contiguous())
    return maps


def set_map(maps, o, y, x, a):
    maps[o][0, :, y, x] = torch.tensor(a, dtype=torch.float32)


def grid(y0, x0, ny, nx, step=3):
    """pixels of an ny x nx grid in pixel order; step 3: no two share a 3 x 3 neighbourhood"""
    return [(y0 + step * i, x0 + step * j) for i in range(ny) for j in range(nx)]


def _unit(shape, sigma):
    """3 s: the half extent of the x 3.0 frame per unit of |a|, in normalised units"""
    return 3.0 * float(sigma) / float(min(shape))


def offdiag():
    """96 x 160, two octaves: isolated maxima well inside the image in every detection level of octave 0 and in two of octave 1; at each
    of them all four map entries are non-zero, distinct and different from every other maximum's.  Nothing is filtered: the rows pin
    the plane and octave indexing of the emit."""
    H, W = 96, 160
    shapes, _ = plan_of(H, W)
    assert shapes == [(96, 160), (48, 80)]
    maps, plant = base_maps(shapes), {}
    pts = {(0, 1): [(40, 60), (40, 90), (55, 75)], (0, 2): [(48, 100), (30, 70)], (0, 3): [(48, 80), (44, 106)],
           (1, 1): [(20, 30), (24, 44), (28, 38)], (1, 2): [(22, 50), (26, 34)]}
    i = 0
    for (o, l), pp in sorted(pts.items()):
        for (y, x) in pp:
            a = (1.25 + i / 32.0, -0.5 - i / 64.0, 0.75 + i / 128.0, 0.875 - i / 32.0) if o == 0 else \
                (0.875 - i / 64.0, 0.625 + i / 128.0, -0.375 - i / 64.0, 1.125 + i / 32.0)
            pl.add_points(plant, shapes[o], (o, l), [(y, x, 10.0 + 1.5 * ((7 * i) % 12))])
            set_map(maps, o, y, x, a)
            i += 1
    return Planted(pl.Case("onepass offdiag 96x160", H, W, plant, {}), maps)


BOUNDARY_DELTA = 0.005           # how far, in normalised units, the deciding corner of a boundary frame lies from the image edge
# name -> (edge, kind): the frame of "<name> out" has exactly ONE corner outside, through the named inequality; "<name> in" is its twin
BOUNDARY_EDGES = {"left": "ox<0", "right": "ox>1", "top": "oy<0", "bottom": "oy>1", "a12 only": "ox>1", "a21 only": "oy>1"}


BOUNDARY_SPOTS = {"left": [(20, 8), (32, 8)], "right": [(20, 87), (32, 87)], "top": [(8, 30), (8, 44)], "bottom": [(55, 30), (55, 44)],
                  "a12 only": [(44, 87), (50, 87)], "a21 only": [(55, 58), (55, 70)]}          # name -> pixels (y, x) of ("out", "in")


def boundary():
    """64 x 96, one octave, pyramid level 2: per image edge one maximum whose x 3.0 frame has exactly one corner outside (by
    BOUNDARY_DELTA) and a twin whose corner is inside by as much; `a12 only` / `a21 only`: the off-diagonal entry alone carries the corner
    across (with a12 = 0 resp. a21 = 0 the frame would be inside by 2 BOUNDARY_DELTA)."""
    H, W = 64, 96
    shapes, sigmas = plan_of(H, W)
    assert shapes == [(64, 96)]
    maps, plant = base_maps(shapes), {}
    u, d = _unit(shapes[0], sigmas[0][2]), BOUNDARY_DELTA
    v = 20.0
    for name, pair in BOUNDARY_SPOTS.items():
        edge = BOUNDARY_EDGES[name]
        for (y, x), state in zip(pair, ("out", "in")):
            cx, cy = (x + 0.5) / W, (y + 0.5) / H
            e = {"ox<0": cx, "ox>1": 1.0 - cx, "oy<0": cy, "oy>1": 1.0 - cy}[edge]          # distance of the centre from its edge
            shift = 0.0 if state == "out" else -2.0 * d
            if name.endswith("only"):        # main term alone: inside by 2 d; with the off-diagonal term: e + d (out) / e - d (in)
                main, off = (e - 2.0 * d) / u, (3.0 * d + shift) / u
            else:                            # main + off = e + d (out) / e - d (in); main - off stays inside
                main, off = (e + shift) / u, d / u
            sgn = -1.0 if name in ("right", "a12 only", "a21 only") else 1.0               # which of the two corners of that edge it is
            a = (main, sgn * off, INSIDE_A[2], INSIDE_A[3]) if edge.startswith("ox") else (INSIDE_A[0], INSIDE_A[1], sgn * off, main)
            assert max(abs(t) for t in a) <= 2.0
            pl.add_points(plant, shapes[0], (0, 2), [(y, x, v)])
            set_map(maps, 0, y, x, a)
            v += 1.25
    return Planted(pl.Case("onepass boundary 64x96", H, W, plant, {}), maps)


def _scatter(vals, n_out, seed):
    """values for a list of pixels in pixel order: the n_out largest go to the first n_out pixels (the ones the builders push outside),
    the rest are shuffled, so that response order and pixel order differ"""
    vals = sorted([float(v) for v in vals], reverse=True)
    rest = vals[n_out:]
    perm = torch.randperm(len(rest), generator=pl._gen(seed)).tolist()
    return vals[:n_out] + [rest[i] for i in perm]


CUT_P, CUT_OUT = 40, 8
NEG_PIXEL = (48, 60)


def cut_level(level, nlevels, n=CUT_P, n_out=CUT_OUT, v0=100.0, a=INSIDE_A, seed=5):
    """64 x 96, one octave: pyramid level `level` holds n positive maxima v0 + i (n_pos = n); the n_out largest sit in the left quarter
    with OUT_LEFT maps, so the filter drops them.  From level 2 up the level also holds ONE negative row at NEG_PIXEL (the octaveMap of a
    lower level acted there: level 2 shares the value 2.5 with level 1, later levels get 7.25 over a 2.0 in level 1) - only an uncut level
    keeps it.  Ballast in every other level."""
    H, W = 64, 96
    shapes, _ = plan_of(H, W, nlevels)
    assert shapes == [(64, 96)] and 1 <= level <= nlevels
    maps, plant = base_maps(shapes, a), {}
    pix = grid(14, 8, 2, 4) + grid(14, 32, 4, 8)                           # the first 8 in the left quarter: x <= 17
    assert len(pix) == n_out + 32 and n <= len(pix)
    pix = pix[:n]
    for (y, x), v in zip(pix, _scatter([v0 + i for i in range(n)], n_out, seed)):
        pl.add_points(plant, shapes[0], (0, level), [(y, x, v)])
    for (y, x) in pix[:n_out]:
        set_map(maps, 0, y, x, OUT_LEFT)
    if level == 2:
        pl.add_points(plant, shapes[0], (0, 1), [NEG_PIXEL + (2.5,)])
        pl.add_points(plant, shapes[0], (0, 2), [NEG_PIXEL + (2.5,)])
    elif level > 2:
        pl.add_points(plant, shapes[0], (0, 1), [NEG_PIXEL + (2.0,)])
        pl.add_points(plant, shapes[0], (0, level), [NEG_PIXEL + (7.25,)])
    pl.add_ballast(plant, shapes[0], [l for l in range(1, nlevels + 1) if l != level])
    return pl.Case("onepass cut level %d nlevels %d n %d" % (level, nlevels, n), H, W, plant, {"nlevels": nlevels}), maps


def cut_switch(level, nlevels):
    """n_pos = CUT_P in pyramid level `level` ("last" = nlevels): the budgets CUT_P - 1 (cut), CUT_P and CUT_P + 1 (no cut) sit around the
    switch `N < n_pos`.  CNT_POS0 of that level comes from hessian_nms_kernel (level 1), resolve_apply_kernel (nlevels 3) or
    level_resolve_kernel (nlevels 4)."""
    return Planted(*cut_level(nlevels if level == "last" else level, nlevels))


COUNTS_N = 40
COUNTS_DRIVERS = {"below": [1.0, 2.0, 3.7], "above": [2.0]}       # level-1 values under three / one of the level-3 maxima


def cut_counts_positives(variant):
    """64 x 96: pyramid level 3 holds COUNTS_N + 2 raw maxima; the octaveMap left by level 1 turns three of them into one zero and two
    negative rows ("below": n_pos = N - 1, no cut, the negative rows stay) or one into a negative row ("above": n_pos = N + 1, cut, it
    goes).  Ten of the largest are pushed outside, so that the global budget does not hide what the level did."""
    H, W = 64, 96
    shapes, _ = plan_of(H, W)
    maps, plant = base_maps(shapes), {}
    pix = grid(14, 8, 2, 5) + grid(14, 32, 4, 8)
    assert len(pix) == COUNTS_N + 2
    vals = _scatter([50.0 + i for i in range(len(pix))], 10, 9)
    for (y, x), v in zip(pix, vals):
        pl.add_points(plant, shapes[0], (0, 3), [(y, x, v)])
    for (y, x) in pix[:10]:
        set_map(maps, 0, y, x, OUT_LEFT)
    for (y, x), v in zip(pix[15::9], COUNTS_DRIVERS[variant]):
        pl.add_points(plant, shapes[0], (0, 1), [(y, x, v)])
    pl.add_ballast(plant, shapes[0], [1, 2])
    return Planted(pl.Case("onepass cut counts positives %s" % variant, H, W, plant, {}), maps)


BEFORE_N = 40


def cut_before_filter():
    """96 x 160, two octaves: pyramid level 2 of octave 0 holds BEFORE_N + 6 positives, the five largest with frames outside: the level
    yields N - 5 rows, the rows ranked N + 1 .. N + 6 are NOT promoted.  Level 3 of octave 0 (3 rows) and level 2 of octave 1 (2 rows) stay
    uncut in the same run, with responses below the cut level's threshold: read through a wrong table entry they would vanish."""
    H, W = 96, 160
    shapes, _ = plan_of(H, W)
    assert shapes == [(96, 160), (48, 80)]
    maps, plant = base_maps(shapes), {}
    pix = grid(30, 10, 1, 5) + grid(36, 60, 5, 9)
    assert len(pix) == BEFORE_N + 10
    pix = pix[:BEFORE_N + 6]
    for (y, x), v in zip(pix, _scatter([100.0 + i for i in range(len(pix))], 5, 13)):
        pl.add_points(plant, shapes[0], (0, 2), [(y, x, v)])
    for (y, x) in pix[:5]:
        set_map(maps, 0, y, x, OUT_LEFT)
    pl.add_points(plant, shapes[0], (0, 3), [(70, 40, 3.0), (70, 80, 4.0), (74, 120, 5.0)])
    pl.add_points(plant, shapes[1], (1, 2), [(20, 30, 1.0), (24, 44, 2.0)])
    return Planted(pl.Case("onepass cut before filter 96x160", H, W, plant, {}), maps)


RADIX_OUT = 8
# (kind, maxima pushed outside, budget; None: first_byte_edge_budget) of every radix run
RADIX_RUNS = [("first", RADIX_OUT, 50), ("first", RADIX_OUT, None), ("first", 0, 1), ("last", RADIX_OUT, 50), ("bucket0", RADIX_OUT, 31),
              ("bucket0", RADIX_OUT, 34), ("all equal", RADIX_OUT, 25)]
RADIX_TIES = {("last", 50), ("bucket0", 31), ("all equal", 25)}           # the cut falls inside a group of equal responses: ties > need
RADIX_EXACT_TIES = {("bucket0", 34)}                                      # ties == need: the whole group is taken


def radix_values(kind):
    """the positive values of the radix level, largest first"""
    if kind == "first":         # about fifteen first bytes (sign + 7 exponent bits: one per factor 4)
        v = pl.log_uniform(1e-3, 1e6, 71)(120)
    elif kind == "last":                         # 1024 + k 2^-13: only the last byte of the key differs; 32 distinct k, the largest eight unique
        k = torch.cat([torch.arange(248, 256), torch.randint(0, 30, (112,), generator=pl._gen(72)) * 8])
        v = (1024.0 + k.double() * 2.0 ** -13).float()
    elif kind == "bucket0":
        # 20 values above 4096; 24, 16, 12 (first byte of 8.0, another third byte); 8 + k 2^-20, k = 1..5 (the bytes of 8.0 but the
        # last); six times 8.0 (every byte below the first is zero: bucket 0 of bytes 2, 1 and 0); powers of two and others below
        v = torch.tensor([4096.0 + 3 * j for j in range(20)] + [24.0, 16.0, 12.0] + [8.0 + k * 2.0 ** -20 for k in range(1, 6)] + [8.0] * 6
                         + [4.0, 2.0, 1.0, 0.5] + [0.1 + 0.37 * j for j in range(12)])
    else:
        v = torch.full((60,), 700.0)
    return torch.sort(v.float(), descending=True)[0]


def radix(kind, n_out=RADIX_OUT):
    """64 x 96, pyramid level 3: radix_values(kind) on a spacing-3 grid; the n_out largest on the first n_out pixels with frames outside
    (the level's cut then shows in the row count: the budget is not refilled).  Two more maxima of the level are turned negative by the
    octaveMap of level 1 (they sit in the select's histogram below every positive key); ballast in levels 1 and 2."""
    H, W = 64, 96
    shapes, _ = plan_of(H, W)
    maps, plant = base_maps(shapes), {}
    vals = radix_values(kind)
    pix = grid(14, 8, 14, 9) if len(vals) > 100 else grid(14, 8, 7, 9)
    assert len(pix) >= len(vals) + 2
    neg = [pix[len(vals)], pix[len(vals) + 1]]
    pix = pix[:len(vals)]
    for (y, x), v in zip(pix, _scatter(vals.tolist(), n_out, 17)):
        pl.add_points(plant, shapes[0], (0, 3), [(y, x, v)])
    for (y, x) in pix[:n_out]:
        assert x <= 32
        set_map(maps, 0, y, x, OUT_LEFT)
    for (y, x), d, v in zip(neg, (2.0, 3.7), (7.25, 9.5)):
        pl.add_points(plant, shapes[0], (0, 1), [(y, x, d)])
        pl.add_points(plant, shapes[0], (0, 3), [(y, x, v)])
    pl.add_ballast(plant, shapes[0], [1, 2])
    return Planted(pl.Case("onepass radix %s out %d" % (kind, n_out), H, W, plant, {}), maps)


def first_byte_edge_budget(rows):
    """kind "first": the budget at which the cut of the radix level coincides with a boundary between two first bytes of the key - the
    first pass of the select meets hist[d] == need"""
    r = rows["resp"][(rows["ids"][:, 1] == 2) & (rows["resp"] > 0)]
    b = np.sort(np.ascontiguousarray(r).view(np.uint32) >> 24)[::-1]
    edges = [i for i in range(20, len(b) - 20) if b[i - 1] != b[i]]
    return edges[len(edges) // 2]


BATCH_N = CUT_P - 1


def batch3():
    """Three constant images 0, 1, 2.  Image 0: cut_level(2, 3) - n_pos = 40, cut by N = 39; image 1: the same level with 30 positives
    50 + i (not cut; under image 0's threshold every one of them would go) and other maps; image 2: image 0 again."""
    c0, m0 = cut_level(2, 3)
    c1, m1 = cut_level(2, 3, n=30, v0=50.0, a=(0.1875, 0.0625, -0.05, 0.25), seed=6)
    return [Planted(c0, m0), Planted(c1, m1), Planted(c0, m0)]


# ---- the runs ------------------------------------------------------------------------------------------------------------------------------
_ROWS = {}


def rows_of(p, value=0.0):
    """level_rows of a case: computed once per process, shared by every budget and test, never modified"""
    key = (p.case.name, value)
    if key not in _ROWS:
        _ROWS[key] = level_rows(p, value)
    return _ROWS[key]


def radix_budget(kind, n_out, N):
    return first_byte_edge_budget(rows_of(radix(kind, n_out))) if N is None else N


def all_runs():
    """[(label, Planted, N, constant image value)]: every (case, budget) that the host tests check against the oracle and the GPU tests
    run through the kernels"""
    runs = [("offdiag", offdiag(), N, 0.0) for N in (100, 4)]
    runs.append(("boundary", boundary(), 100, 0.0))
    for level in (1, 2, "last"):
        for nlevels in (3, 4):
            runs += [("cut_switch %s/%d" % (level, nlevels), cut_switch(level, nlevels), CUT_P + d, 0.0) for d in (-1, 0, 1)]
    runs += [("cut_counts_positives " + v, cut_counts_positives(v), COUNTS_N, 0.0) for v in ("below", "above")]
    runs.append(("cut_before_filter", cut_before_filter(), BEFORE_N, 0.0))
    runs += [("radix %s" % kind, radix(kind, n_out), radix_budget(kind, n_out, N), 0.0) for kind, n_out, N in RADIX_RUNS]
    runs += [("batch3 image %d" % b, p, BATCH_N, float(b)) for b, p in enumerate(batch3())]
    return runs


ALL_RUNS = all_runs()
RUN_IDS = ["%s N=%d" % (r[0], r[2]) for r in ALL_RUNS]
