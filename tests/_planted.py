"""Planted response pyramids (host only: torch CPU + the oracle, no GPU import).

Everything behind the Hessian response in the detector is discrete decision logic: 3-D NMS with its +1e-5 slack, the border rule, the
uint8 octaveMap replay with its wrap and the negative rows it produces, the "<= 1 positive: skip the level" rule, the global top-C
select, the tie cut and the rank sort.  The RespNet slot is any callable(level, sigma) on both sides (OracleExtractor(resp_fn=...),
ScaleSpaceAffinePatchExtractor(RespNet=...)), so a test can hand both the SAME hand-built response pyramid on an all-zero image and
demand the oracle's rows key for key and bit for bit.  This module builds such pyramids and turns the oracle's keep-all rows into what
the detector must return for a feature budget N.

tests/test_planted_oracle.py proves on the oracle alone that every construction below reaches the branch it is named after;
tests/test_gpu_planted_responses.py runs them through the kernels.
"""
import collections

import numpy as np
import torch

import affnet_oracle as orc

MR, BORDER = 5.192, 5            # the detector configuration every planted case uses (border rule: int(mrSize) = 5 px)


def plan_of(H, W, nlevels=3, init_sigma=1.6, border=BORDER):
    """([(h, w) per octave], [level sigmas per octave]) of an H x W image: HandCraftedModules.py:14-56 through the oracle's plan."""
    octs = orc.pyramid_plan(H, W, nlevels, init_sigma, border)["octaves"]
    return [(o["h"], o["w"]) for o in octs], [list(o["level_sigmas"]) for o in octs]


def planted_fn(H, W, plant, sigmas):
    """A fresh callable fn(level (1,1,h,w), sigma) -> plant[(octave, pyramid level)] or zeros of the level's shape.  The octave is read off
    the level's shape, the pyramid level off `sigma` in that octave's sigma list (`sigmas`: per octave, as plan_of / the GPU plan give
    them): nothing depends on the order of the calls, which differs between the two sides."""
    shapes, (h, w) = [], (int(H), int(W))
    for _ in sigmas:
        shapes.append((h, w))
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert len(set(shapes)) == len(shapes)
    for (o, l), m in plant.items():
        assert tuple(m.shape) == (1, 1) + shapes[o] and m.dtype == torch.float32 and 0 <= l < len(sigmas[o]), (o, l, tuple(m.shape))

    def fn(level, sigma):
        hw = (int(level.shape[2]), int(level.shape[3]))
        o = shapes.index(hw)
        d = [abs(float(s) - float(sigma)) for s in sigmas[o]]
        l = int(np.argmin(d))
        assert d[l] <= 1e-6 * float(sigma), "sigma %r is not a level of octave %d" % (sigma, o)
        m = plant.get((o, l))
        return torch.zeros(1, 1, hw[0], hw[1]) if m is None else m.clone()
    return fn


# ---- reference rows ------------------------------------------------------------------------------------------------------------------------
def oracle_rows(H, W, plant, nlevels=3, th=None, **kw):
    """The reference's keep-all rows for the planted pyramid, in its concatenation order (octave, level, pixel):
    dict(ids (n,3) int64 = (octave, detection level, flat pixel), resp (n,) fp32, lafs (n,2,3) fp32 pixels)."""
    ex = orc.OracleExtractor(mrSize=MR, border=BORDER, num_features=-1, num_Baum_iters=0, nlevels=nlevels, th=th,
                             resp_fn=planted_fn(H, W, plant, plan_of(H, W, nlevels)[1]), **kw)
    L, r = ex(torch.zeros(1, 1, H, W))
    return {"ids": ex.keys.numpy().astype(np.int64), "resp": r.numpy().copy(), "lafs": L.numpy().copy()}


def order_key(ids):
    return (ids[:, 0].astype(np.int64) << 40) | (ids[:, 1].astype(np.int64) << 32) | ids[:, 2].astype(np.int64)


def select_rows(rows, N):
    """What the detector must return for num_features = N given the reference's keep-all rows: more than N rows -> the first N under
    (response descending, (octave, level, pixel) ascending), in that order (SparseImgRepresenter.py:104-109 is a torch.topk, whose choice
    among equal values is unspecified: the key order is this project's rule); otherwise every row in (octave, level, pixel) order."""
    k = order_key(rows["ids"])
    n = len(k)
    if 0 < N < n:
        sel = np.lexsort((k, -rows["resp"].astype(np.float64)))[:N]
    else:
        sel = np.argsort(k, kind="stable")
    return {"ids": rows["ids"][sel], "resp": rows["resp"][sel], "lafs": rows["lafs"][sel]}


def expected_rows(H, W, plant, N, **kw):
    return select_rows(oracle_rows(H, W, plant, **kw), N)


# ---- builders ------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def uniform(lo, hi, seed):
    """value generator: n fp32 values uniform in [lo, hi)"""
    g = _gen(seed)
    return lambda n: (lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)).float()


def log_uniform(lo, hi, seed):
    g = _gen(seed)
    return lambda n: torch.exp(np.log(lo) + (np.log(hi) - np.log(lo)) * torch.rand(n, generator=g, dtype=torch.float64)).float()


def quantised(base, step, count, seed):
    """value generator: base + k * step for random integer k < count (exact in fp32 when the caller picks step = ulp(base))"""
    g = _gen(seed)
    return lambda n: (base + step * torch.randint(0, count, (n,), generator=g).double()).float()


def lattice(shape, step, offset, values):
    """(1,1,h,w) map, zero except on the pixels (offset + i step, offset + j step); `values`: a number or a generator(n) -> (n,) fp32."""
    h, w = shape
    m = torch.zeros(1, 1, h, w)
    ny, nx = len(range(offset, h, step)), len(range(offset, w, step))
    v = values(ny * nx) if callable(values) else torch.full((ny * nx,), float(values))
    m[0, 0, offset::step, offset::step] = v.view(ny, nx)
    return m


def add_points(plant, shape, key, pts):
    m = plant.setdefault(key, torch.zeros(1, 1, shape[0], shape[1]))
    for y, x, v in pts:
        assert float(m[0, 0, y, x]) == 0.0
        m[0, 0, y, x] = v
    return plant


def add_ballast(plant, shape, levels, octave=0, row=6, base=0.0625):
    """Two isolated small maxima per listed pyramid level of `octave`, so that the "<= 1 positive -> the level is skipped" rule
    (HandCraftedModules.py:252-254) fires only where a case plants it.  Level l's pair sits on `row` at x = 6 + 8 (l - 1) and 4 px
    further right: no two ballast points share a 3 x 3 x 3 neighbourhood, and the builder asserts that nothing else is planted in
    theirs.  Values base (1 + i / 16), all different."""
    h, w = shape
    i = 0
    for l in levels:
        for x in (6 + 8 * (l - 1), 10 + 8 * (l - 1)):
            assert BORDER <= row < h - BORDER and BORDER <= x < w - BORDER, (shape, l, x)
            for ll in (l - 1, l, l + 1):
                m = plant.get((octave, ll))
                assert m is None or float(m[0, 0, row - 1:row + 2, x - 1:x + 2].abs().sum()) == 0.0, "ballast is not isolated"
            add_points(plant, shape, (octave, l), [(row, x, base * (1.0 + i / 16.0))])
            i += 1
    return plant


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name H W plant kw")      # kw: oracle / extractor keywords that differ from the defaults (nlevels, th)


def single_bucket(H, W, kind):
    """Spacing-3 lattice at offset 1 in pyramid level 2 of octave 0, every value inside one first-digit bucket of the radix select (order
    key bits 31..21 = sign, exponent, two mantissa bits: [1024, 1280)).  kind "digit3": 1024 + k 2^-13 (one ulp), k < 1024 - digits 1 and 2
    shared, the third decides alone and every value is tied about twenty times; kind "digit2": uniform in [1024, 1279)."""
    shapes, _ = plan_of(H, W)
    values = quantised(1024.0, 2.0 ** -13, 1024, 21) if kind == "digit3" else uniform(1024.0, 1279.0, 22)
    return Case("bucket %s %dx%d" % (kind, H, W), H, W, {(0, 2): lattice(shapes[0], 3, 1, values)}, {})


def dense_tiles():
    """48 x 128: spacing-2 lattices, offset 0 in pyramid level 1 and offset 1 in level 3, values in [1, 900): every 64 x 16 tile of octave 0
    holds more maxima than the NMS kernel's staging list (HN_CAP)."""
    H, W = 48, 128
    shapes, _ = plan_of(H, W)
    return Case("dense tiles 48x128", H, W, {(0, 1): lattice(shapes[0], 2, 0, uniform(1.0, 900.0, 31)),
                                            (0, 3): lattice(shapes[0], 2, 1, uniform(1.0, 900.0, 32))}, {})


def all_equal():
    """96 x 128: 700.0 on spacing-3 lattices in two levels of each of two octaves: one response value, the order keys alone decide."""
    H, W = 96, 128
    shapes, _ = plan_of(H, W)
    return Case("all equal 96x128", H, W, {(0, 1): lattice(shapes[0], 3, 0, 700.0), (0, 3): lattice(shapes[0], 3, 1, 700.0),
                                           (1, 1): lattice(shapes[1], 3, 0, 700.0), (1, 2): lattice(shapes[1], 3, 1, 700.0)}, {})


STACK_PIXEL = (24, 100)
STACK_VALUES = (0.75, 1.5, 2.5, 300.25)
# detection level -> response at STACK_PIXEL (the octaveMap replay by hand: m = uint8(int64(m + v (1 - m))) after every applied level)
STACK_ROWS = {0.75: [(0, 0.75), (1, 0.75), (2, 0.75)], 1.5: [(0, 1.5)], 2.5: [(0, 2.5), (1, -2.5), (2, 2.5)],
              300.25: [(0, 300.25), (1, -12910.75), (2, -56747.25)]}


def stack(v, nlevels):
    """48 x 128: one pixel carries the value v in pyramid levels 1, 2 and 3 (the slack keeps all three in the NMS; the octaveMap decides what
    is left of levels 2 and 3), ballast in every detection level."""
    H, W = 48, 128
    shapes, _ = plan_of(H, W, nlevels)
    plant = {}
    for l in (1, 2, 3):
        add_points(plant, shapes[0], (0, l), [STACK_PIXEL + (v,)])
    add_ballast(plant, shapes[0], range(1, nlevels + 1))
    return Case("stack v=%g nlevels=%d" % (v, nlevels), H, W, plant, {"nlevels": nlevels})


WRAP_VALUES = [0.5, 0.999, 1.0, 1.5, 2.0, 3.7, 255.9, 256.0, 256.5, 257.0, 511.9, 512.5, 1024.25, 1025.0]
WRAP_ABSENT = [1.0, 1.5, 257.0, 1025.0]          # uint8(int64(v)) == 1: the level-3 response is multiplied by 1 - 1
WRAP_ROW, WRAP_X0, WRAP_TOP = 20, 8, 7.25


def wrap_table(nlevels):
    """64 x 80: the level-1 values of WRAP_VALUES (x = 8, 12, ...), each under a level-3 maximum of 7.25 at the same pixel."""
    H, W = 64, 80
    shapes, _ = plan_of(H, W, nlevels)
    plant = {}
    for i, v in enumerate(WRAP_VALUES):
        add_points(plant, shapes[0], (0, 1), [(WRAP_ROW, WRAP_X0 + 4 * i, v)])
        add_points(plant, shapes[0], (0, 3), [(WRAP_ROW, WRAP_X0 + 4 * i, WRAP_TOP)])
    add_ballast(plant, shapes[0], range(1, nlevels + 1))
    return Case("wrap table nlevels=%d" % nlevels, H, W, plant, {"nlevels": nlevels})


SLACK_NEAR = float(np.float32(5.0) + np.float32(4e-6))       # 8 ulp above 5.0: inside the +1e-5 slack
SLACK_FAR = float(np.float32(5.0) + np.float32(2e-5))
SLACK_PIXELS = {"near_lo": (20, 30), "near_hi": (20, 31), "far_lo": (30, 60), "far_hi": (31, 61)}


def slack(nlevels):
    """48 x 128, pyramid level 2: horizontal neighbours 5.0 and 5.0 + 4e-6 (both survive `x - max + 1e-5 > 0`), diagonal neighbours 5.0 and
    5.0 + 2e-5 (only the larger does)."""
    H, W = 48, 128
    shapes, _ = plan_of(H, W, nlevels)
    P = SLACK_PIXELS
    plant = add_points({}, shapes[0], (0, 2), [P["near_lo"] + (5.0,), P["near_hi"] + (SLACK_NEAR,), P["far_lo"] + (5.0,), P["far_hi"] + (SLACK_FAR,)])
    add_ballast(plant, shapes[0], range(1, nlevels + 1))
    return Case("slack nlevels=%d" % nlevels, H, W, plant, {"nlevels": nlevels})


SKIP_ONE, SKIP_TWO = [(20, 30, 9.0)], [(20, 30, 9.0), (30, 90, 13.0)]


def skip_rule(nlevels):
    """48 x 128: pyramid level 1 holds exactly ONE positive maximum (the level yields no row and leaves the octaveMap alone), level 2
    exactly two (both rows) - one of them on the pixel of level 1's maximum with the same value: had level 1 been applied, the octaveMap
    (9) would turn it into -72 and level 2 would be down to one positive.  Ballast only from level 3 up."""
    H, W = 48, 128
    shapes, _ = plan_of(H, W, nlevels)
    plant = add_points({}, shapes[0], (0, 1), SKIP_ONE)
    add_points(plant, shapes[0], (0, 2), SKIP_TWO)
    add_ballast(plant, shapes[0], range(3, nlevels + 1))
    return Case("skip rule nlevels=%d" % nlevels, H, W, plant, {"nlevels": nlevels})


def seams(H, W):
    """Spacing-3 lattices in every octave: offset 0 in pyramid level 1, offset 1 in level 2, offset 2 in level 3, values in [1, 900).
    Together the offsets put maxima on both sides of every 64-column / 16-row tile seam and into the partial tiles at the right and
    bottom edge; lattice points of adjacent levels are diagonal neighbours, so the 3-D NMS decides between them (which of them survive
    depends on the values: tests/test_planted_oracle.py asserts that the survivors of these seeds still cover every seam)."""
    shapes, _ = plan_of(H, W)
    plant = {}
    for o, s in enumerate(shapes):
        for off in (0, 1, 2):
            plant[(o, 1 + off)] = lattice(s, 3, off, uniform(1.0, 900.0, 100 * o + off + 46))
    return Case("seams %dx%d" % (H, W), H, W, plant, {})


def wide_range():
    """192 x 256: spacing-3 lattice in pyramid level 2, values log-uniform over 1e-3 .. 1e6 (about thirty first-digit buckets per decade)."""
    H, W = 192, 256
    shapes, _ = plan_of(H, W)
    return Case("log-uniform 192x256", H, W, {(0, 2): lattice(shapes[0], 3, 1, log_uniform(1e-3, 1e6, 51))}, {})


def one_lattice():
    """48 x 128: one spacing-3 lattice of distinct-ish values in pyramid level 2: the budget is set to n - 1, n and n + 1 of its n rows."""
    H, W = 48, 128
    shapes, _ = plan_of(H, W)
    return Case("one lattice 48x128", H, W, {(0, 2): lattice(shapes[0], 3, 1, uniform(1.0, 900.0, 61))}, {})


TH = 3.3
TH_NEXT = float(np.nextafter(np.float32(3.3), np.float32(4.0)))
TH_POINTS = [(20, 30, 3.2), (20, 50, float(np.float32(3.3))), (20, 70, TH_NEXT), (20, 90, 5.0)]


def threshold_mode():
    """48 x 128, th = 3.3: level-2 values 3.2, 3.3 (both clamp to zero), the next float above 3.3 (survives with 2.4e-7) and 5.0; ballast
    above the threshold in every level."""
    H, W = 48, 128
    shapes, _ = plan_of(H, W)
    plant = add_points({}, shapes[0], (0, 2), TH_POINTS)
    add_ballast(plant, shapes[0], range(1, 4), base=4.0)
    return Case("threshold mode th=3.3", H, W, plant, {"th": TH})
