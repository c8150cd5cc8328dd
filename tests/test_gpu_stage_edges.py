"""GPU (run with -m gpu on an MI355X): the three detector-side stage kernels at the shapes where their dispatch and edge logic decide,
against the host-independent fp32 mirrors of tests/_fp32_chain.py (pinned on the CPU by tests/test_fp32_chain_host.py).  The kernels
claim to replay the reference's fp32 operation sequence, so EVERY comparison is exact (np.array_equal over every element: no mask, no
percentile, no tolerance); torch is not the reference here (its CPU conv2d is not the fmaf chain for 3 x 3 kernels on small inputs, and
affine_grid rounds differently from host to host).

Blur (csrc/pyramid.hip).  Dispatch arithmetic restated below (blur_bt_r, pair_bt_r, pyramid_launches): a single blur takes BT_R = 4
(64 x 64 tiles) iff cdiv(w, 64) * cdiv(h, 64) * batch >= 1024, else BT_R = 1 (64 x 16 tiles); the paired launch of (last level of octave
o, level 1 of octave o + 1) - taken for 15 / 9 taps - decides on the SUM of both jobs' 64 x 64 tile counts; a row is stored as float4 iff
w % 4 == 0, x + 3 < w and the level's base address is 16-byte aligned, else by the scalar loop; the blur of level n_levels also writes
the next octave's level 0 (fused stride-2 decimation, packed in the float4 branch, per pixel in the scalar one).

  case                                          taps        BT_R  store            decimation        pair kernel
  test_blur_every_tap_size         21 x 70      1 .. 37     1     scalar           -                 -
  test_blur_tile_geometry          1x1 .. 33x132  3 9 15 37 1     scalar + float4  -                 -
  test_blur_throughput_shape  52 x (193 x 257)  11 9 11 13  4     scalar           scalar, BT_R 4    <15, 9, 4>: octave 1 level 1 in BT_R 4
                              (octaves >= 1)    11 13 15 9  1     scalar           scalar, BT_R 1    <15, 9, 1>
                              64 x (256 x 256)  11 9 11 13  4     float4           packed, BT_R 4    <15, 9, 4>
                              (octaves >= 1)    11 13 15 9  1     float4           packed, BT_R 1    <15, 9, 1>
                  nlevels 1:  52 x (193 x 257)  11 17 35    4     scalar           scalar, BT_R 4    not taken (35 / 17 taps: two launches)
  test_pyramid_pair_and_decimation_parities     11 9 .. 15  1     both             both, odd + even  <15, 9, 1>, batch 1 and 3
      64 x 64, 65 x 129, 66 x 130, 127 x 61, 61 x 128 (h x w): the levels that are decimated cover every (h, w) parity, widths with
      w % 4 == 0 (float4 store + packed decimation, also at an odd height) and != 0; all far below 1024 tiles -> BT_R 1

Each of these statements is ASSERTED in the test that relies on it, from the restated arithmetic, so a changed threshold in the source
shows up as a failing coverage assertion and not as a silently narrower test.

Hessian (hessian_resp_kernel, 64 x 4 tiles), detector (hessian_nms_kernel, 64 x 16 tiles) at tile-exact / tile-plus-one sizes.
Sampler (grid_sample_kernel): frames stepped across the staged / direct boundary tw * th <= min(4096, 2 ps^2) of aff_tile_box, boxes
with negative origins, overhanging and outside frames, and the pyramid entry point with a batch, per-image counts and id clamping."""
import ctypes as C

import numpy as np
import pytest
import torch

import affnet_oracle as orc
import _fp32_chain as fc
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return affnet_amd


def cdiv(a, b):
    return (a + b - 1) // b


# ---- csrc/pyramid.hip dispatch, restated -------------------------------------------------------------------------------------------
def blur_bt_r(h, w, batch):
    """launch_blur: the throughput shape needs >= 1024 tiles of 64 x 64."""
    return 4 if cdiv(w, 64) * cdiv(h, 64) * batch >= 1024 else 1


def pair_bt_r(ha, wa, hb, wb, batch):
    """launch_blur_pair: one decision for both jobs, on the sum of their 64 x 64 tile counts."""
    return 4 if (cdiv(wa, 64) * cdiv(ha, 64) + cdiv(wb, 64) * cdiv(hb, 64)) * batch >= 1024 else 1


def taps_of(sigma):
    return int(6.0 * sigma + 1.0) | 1


def pyramid_launches(h, w, batch, n_levels=3, init_sigma=1.6, border=5):
    """(sizes, {(octave, level): how affnet_pyramid_build produces that level}) - the loop of affnet_pyramid_build restated: k taps,
    BT_R, whether the level comes out of the paired launch, whether its blur also decimates, or (level 0 of octave >= 1) that it IS the
    decimation store of the previous octave's level n_levels."""
    first, octs = fc.pyramid_plan(h, w, n_levels, init_sigma, border)
    L = n_levels + 2
    sizes = [(o[0], o[1]) for o in octs]
    out = {(0, 0): dict(k=taps_of(first), bt_r=blur_bt_r(h, w, batch), pair=False, dec=False)}
    for o, (oh, ow, blurs) in enumerate(octs):
        ks = [None] + [taps_of(s) for s in blurs]
        if o > 0:
            out[(o, 0)] = dict(k=out[(o - 1, L - 2)]["k"], bt_r=out[(o - 1, L - 2)]["bt_r"], pair=False, dec=False, decimated_from=(o - 1, L - 2))
        for l in range(1, L):
            if (o, l) in out:                          # level 1 written by the previous octave's paired launch
                continue
            last = o + 1 == len(octs)
            if l == L - 1 and not last and ks[l] == 15 and taps_of(octs[o + 1][2][0]) == 9:
                b = pair_bt_r(oh, ow, sizes[o + 1][0], sizes[o + 1][1], batch)
                out[(o, l)] = dict(k=15, bt_r=b, pair=True, dec=False)
                out[(o + 1, 1)] = dict(k=9, bt_r=b, pair=True, dec=False)
            else:
                out[(o, l)] = dict(k=ks[l], bt_r=blur_bt_r(oh, ow, batch), pair=False, dec=(l == L - 2 and not last))
    return sizes, out


def locate_blur(y, x, h, w, k, bt_r, aligned=True, dec=False):
    """Where pixel (y, x) of an h x w blur output sits in the kernel's tiling."""
    r, th = k // 2, 16 * bt_r
    lx, ly = x % 64, y % th
    halo = [n for n, hit in (("left", lx < r), ("right", lx >= 64 - r), ("top", ly < r), ("bottom", ly >= th - r)) if hit]
    clamp = [n for n, hit in (("left", x < r), ("right", x + r >= w), ("top", y < r), ("bottom", y + r >= h)) if hit]
    vec = (w % 4 == 0) and aligned and ((x & ~3) + 3 < w)
    s = "tile column %d of %d (local x %d, thread column %d lane %d), tile row %d of %d (local y %d) in %d x %d tiles [BT_R %d, %d taps]" % (
        x // 64, cdiv(w, 64), lx, lx // 4, lx % 4, y // th, cdiv(h, th), ly, 64, th, bt_r, k)
    s += "; taps reach the %s halo" % "/".join(halo) if halo else "; taps stay inside the tile"
    s += "; replicate-clamped at the image's %s edge" % "/".join(clamp) if clamp else ""
    s += "; %s store path" % ("float4" if vec else "scalar")
    if dec:
        s += "; %s" % ("a decimated pixel (written to the next octave too)" if (y % 2 == 0 and x % 2 == 0) else "not a decimated pixel")
    return s


def assert_exact(name, got, want, where=None, report=True):
    """np.array_equal over every element; on failure the first differing element and `where(index tuple)` for it."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (name, got.shape, want.shape)
    ne = got != want
    n_bad = int(ne.sum())
    d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    if report or n_bad:
        print("%s: max abs diff %.3g, mismatching elements %d / %d" % (name, d, n_bad, got.size))
        record_parity("stage edges: " + name, max_abs_diff=d, mismatching_elements=n_bad, elements=int(got.size))
    if n_bad:
        idx = tuple(int(v) for v in np.argwhere(ne | np.isnan(got))[0])
        rows = np.argwhere(ne)
        box = "differing elements span %s .. %s" % (rows.min(axis=0).tolist(), rows.max(axis=0).tolist()) if len(rows) else "NaN"
        raise AssertionError("%s: %d of %d elements differ (max %g); first at %s: got %r, want %r; %s; %s" % (
            name, n_bad, got.size, d, idx, got[idx], want[idx], box, where(idx) if where else ""))


# ---- blur: the stand-alone entry point ---------------------------------------------------------------------------------------------
def gpu_blur(x, taps):
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr
    ctx = engine.utility_ctx(torch.device(DEV))
    h, w = x.shape
    k = taps.shape[0]
    xin = torch.from_numpy(np.array(x, dtype=F32)).to(DEV)
    out = torch.full((h, w), SENTINEL, dtype=torch.float32, device=DEV)
    assert out.data_ptr() % 16 == 0
    buf = (C.c_float * (k * k))(*taps.reshape(-1).tolist())
    rc = lib.affnet_gauss_blur(ctx, ptr(xin), ptr(out), h, w, buf, k, None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), ctx


def check_blur(h, w, k, seed):
    x = fc.noise_image(h, w, seed)
    taps = fc.gaussian_taps(fc.sigma_for_taps(k))
    assert taps.shape == (k, k)
    assert blur_bt_r(h, w, 1) == 1
    rc, got, _ = gpu_blur(x, taps)
    assert rc == 0
    assert_exact("blur %d taps on %d x %d (h x w)" % (k, h, w), got, fc.blur_chain_taps(x, taps), lambda i: locate_blur(i[0], i[1], h, w, k, 1))


@pytest.mark.parametrize("k", list(range(1, 38, 2)))
def test_blur_every_tap_size(amd, k):
    """All 19 instantiations in the latency shape on 21 x 70: one full tile column + 6 px, a second tile row of 5 rows, scalar stores."""
    assert 70 % 4 != 0 and cdiv(70, 64) == 2 and cdiv(21, 16) == 2
    check_blur(21, 70, k, 100 + k)


def test_blur_unsupported_tap_size_is_an_error_and_writes_nothing(amd):
    from affnet_amd import _lib
    taps = fc.gaussian_taps(fc.sigma_for_taps(39))
    assert taps.shape == (39, 39)
    rc, out, ctx = gpu_blur(fc.noise_image(21, 70, 39), taps)
    assert rc == _lib.ERR_INVALID and b"39" in _lib.lib.affnet_last_error(ctx)
    assert np.all(out == F32(SENTINEL)), "the refused call wrote to the output"


# 1 x 1, one row, tile-exact, tile + 1, tile - 1, two tile columns on the float4 path, float4 path with a partial last tile column and a
# third tile row of one row; K = the smallest, the two defaults of the paired launch, the largest
GEOMETRY = [(1, 1), (1, 64), (16, 64), (17, 65), (15, 63), (8, 128), (33, 132)]


@pytest.mark.parametrize("k", [3, 9, 15, 37])
@pytest.mark.parametrize("h,w", GEOMETRY, ids=["%dx%d" % s for s in GEOMETRY])
def test_blur_tile_geometry(amd, h, w, k):
    check_blur(h, w, k, 7 * h + w + k)


def test_blur_halo_larger_than_the_image(amd):
    """5 x 4 with 37 taps: every load of the 52 x 100 tile is replicate-clamped (float4 store: 4 % 4 == 0, x + 3 < 4 for x = 0)."""
    check_blur(5, 4, 37, 54)


# ---- blur: the pyramid, batched ----------------------------------------------------------------------------------------------------
_PYR_REF = {}                 # (h, w, seed, n_levels) -> (image, chain pyramid): computed once, shared, read-only


def pyr_ref(h, w, seed, n_levels=3):
    key = (h, w, seed, n_levels)
    if key not in _PYR_REF:
        img = fc.noise_image(h, w, seed)
        pyr = fc.pyramid_chain(img, n_levels, 1.6, 5)
        for arr in [img] + [l for o in pyr for l in o]:
            arr.setflags(write=False)
        _PYR_REF[key] = (img, pyr)
    return _PYR_REF[key]


def build_pyramids(h, w, seeds, n_levels=3):
    """affnet_pyramid_build on a batch whose slot b holds noise_image(h, w, seeds[b]); returns (context, level(b, o, l) reader,
    aligned(b, o, l))."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    B = len(seeds)
    ctx = engine.Context(h, w, dev, n_levels, 1.6, 5, 5.192, 0.0, 60, 60, batch=B)
    x = torch.from_numpy(np.stack([pyr_ref(h, w, s, n_levels)[0] for s in seeds])).to(dev).contiguous()
    check(lib.affnet_pyramid_build(ctx.handle, ptr(x), engine.stream_of(dev)), ctx.handle, "affnet_pyramid_build")
    torch.cuda.synchronize()
    sizes, L = ctx.plan.sizes, ctx.plan.levels_per_octave
    stride = lib.affnet_pyramid_image_stride(ctx.handle)
    off = {(o, l): lib.affnet_pyramid_level_offset(ctx.handle, o, l) for o in range(len(sizes)) for l in range(L)}
    lo = min(off.values())
    hi = (B - 1) * stride + max(off[(o, l)] + sizes[o][0] * sizes[o][1] for (o, l) in off)
    ws = ctx._ws_f32[lo:hi].cpu().numpy()                       # one copy of every image's pyramid
    base = ctx._ws_f32.data_ptr()

    def level(b, o, l):
        s = b * stride + off[(o, l)] - lo
        return ws[s:s + sizes[o][0] * sizes[o][1]].reshape(sizes[o])

    def aligned(b, o, l):
        return (base + 4 * (b * stride + off[(o, l)])) % 16 == 0
    return ctx, level, aligned


def check_pyramids(h, w, seeds, n_levels=3):
    """Every level of every octave of every slot against the chain pyramid of the slot's source image."""
    sizes, how = pyramid_launches(h, w, len(seeds), n_levels)
    ctx, level, aligned = build_pyramids(h, w, seeds, n_levels)
    assert sizes == list(ctx.plan.sizes) and n_levels + 2 == ctx.plan.levels_per_octave
    for b, seed in enumerate(seeds):
        ref = pyr_ref(h, w, seed, n_levels)[1]
        assert len(ref) == len(sizes)
        for o, (oh, ow) in enumerate(sizes):
            for l in range(n_levels + 2):
                hw = how[(o, l)]
                name = "pyramid %d x (%d x %d) nlevels %d: slot %d (image %d) octave %d level %d" % (len(seeds), h, w, n_levels, b, seed, o, l)
                if "decimated_from" in hw:
                    po, pl = hw["decimated_from"]
                    ph, pw = sizes[po]
                    assert np.array_equal(ref[o][0], ref[po][pl][::2, ::2])
                    where = lambda i: "decimation store of octave %d level %d pixel (%d, %d): %s" % (
                        po, pl, 2 * i[0], 2 * i[1], locate_blur(2 * i[0], 2 * i[1], ph, pw, hw["k"], hw["bt_r"], aligned(b, po, pl), True))
                else:
                    where = lambda i: ("paired launch; " if hw["pair"] else "") + locate_blur(i[0], i[1], oh, ow, hw["k"], hw["bt_r"], aligned(b, o, l), hw["dec"])
                assert_exact(name, level(b, o, l), ref[o][l], where, report=False)
    n = len(seeds) * len(sizes) * (n_levels + 2)
    print("pyramid %d x (%d x %d) nlevels %d: %d levels equal the chain" % (len(seeds), h, w, n_levels, n))
    record_parity("stage edges: pyramid %d x (%d x %d) nlevels %d" % (len(seeds), h, w, n_levels), levels_compared=n, mismatching_elements=0,
                  launches={"%d,%d" % k: {a: b for a, b in v.items() if a != "decimated_from"} for k, v in how.items()})
    return sizes, how, aligned


def slot_order(batch):
    """Three source images in a non-repeating order; first, middle and last slot hold different ones."""
    src = np.random.RandomState(batch).randint(0, 3, batch)
    src[0], src[batch // 2], src[-1] = 0, 1, 2
    assert all(np.any(src[p:] != src[:-p]) for p in range(1, 7)), "the slot order repeats with a short period"
    return [int(s) + 1 for s in src]


def test_blur_throughput_shape_odd_size(amd):
    """52 x (193 x 257): 5 x 4 = 20 tiles of 64 x 64 per image, 1040 in all -> BT_R = 4 for octave 0 (first blur, levels 1 .. 3, the
    level-3 blur with the fused scalar decimation at an odd width and height; y >= h in the last tile row: 193 = 3 * 64 + 1).  The paired
    launch (octave 0 level 4 + octave 1 level 1) counts (20 + 6) * 52 = 1352 tiles -> BT_R = 4 for BOTH jobs, although a single blur of
    the 97 x 129 octave 1 (312 tiles) takes BT_R = 1 - as its levels 2 .. 4 then do."""
    B, h, w = 52, 193, 257
    sizes, how, _ = check_pyramids(h, w, slot_order(B))
    assert sizes[:2] == [(193, 257), (97, 129)]
    assert [how[(0, l)]["bt_r"] for l in range(5)] == [4] * 5 and [how[(0, l)]["k"] for l in range(5)] == [11, 9, 11, 13, 15]
    assert how[(0, 3)]["dec"] and how[(0, 4)]["pair"] and how[(1, 1)] == dict(k=9, bt_r=4, pair=True, dec=False)
    assert blur_bt_r(97, 129, B) == 1 and [how[(1, l)]["bt_r"] for l in (2, 3, 4)] == [1, 1, 1] and how[(1, 4)]["pair"]
    assert w % 4 != 0


def test_blur_throughput_shape_float4_and_packed_decimation(amd):
    """64 x (256 x 256): exactly 1024 tiles -> BT_R = 4 at the threshold itself, float4 stores, the packed decimation store."""
    B, h, w = 64, 256, 256
    assert cdiv(w, 64) * cdiv(h, 64) * B == 1024
    sizes, how, aligned = check_pyramids(h, w, slot_order(B))
    assert [how[(0, l)]["bt_r"] for l in range(5)] == [4] * 5 and how[(0, 3)]["dec"] and how[(1, 1)]["bt_r"] == 4 and how[(1, 2)]["bt_r"] == 1
    assert all(aligned(b, o, l) for b in range(B) for o in range(2) for l in range(5)), "a level is not 16-byte aligned: the float4 store path is not reached"
    assert len(sizes) == 5 and sizes[-1] == (16, 16)


def test_blur_throughput_shape_35_taps(amd):
    """nlevels = 1: Gaussians of 11, 17 and 35 taps; 35 / 17 taps do not take the paired launch, so the 35-tap kernel runs alone in
    BT_R = 4 (the largest register window of the throughput shape the default constructor arguments can reach)."""
    B, h, w = 52, 193, 257
    sizes, how, _ = check_pyramids(h, w, slot_order(B), n_levels=1)
    assert [how[(0, l)] for l in range(3)] == [dict(k=11, bt_r=4, pair=False, dec=False), dict(k=17, bt_r=4, pair=False, dec=True),
                                               dict(k=35, bt_r=4, pair=False, dec=False)]


PAIR_SIZES = [(64, 64), (65, 129), (66, 130), (127, 61), (61, 128)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("h,w", PAIR_SIZES, ids=["%dx%d" % s for s in PAIR_SIZES])
def test_pyramid_pair_and_decimation_parities(amd, h, w, batch):
    """Default settings, so every octave but the last ends in blur2d_pair_kernel<15, 9, 1> (at most (3 * 2 + 2 * 1) * 3 = 24 tiles: BT_R = 1
    throughout); the sizes cover odd / even height and width of the level that is decimated and both store paths
    (tests/test_fp32_chain_host.py::test_stage_edge_dispatch_restatement_and_size_coverage)."""
    sizes, how, _ = check_pyramids(h, w, [5, 6, 7][:batch])
    assert len(sizes) >= 3
    assert all(v["bt_r"] == 1 for v in how.values())
    for o in range(len(sizes) - 1):
        assert how[(o, 4)] == dict(k=15, bt_r=1, pair=True, dec=False) and how[(o + 1, 1)] == dict(k=9, bt_r=1, pair=True, dec=False)
        assert how[(o, 3)]["dec"] and how[(o, 3)]["k"] == 13
    assert not how[(len(sizes) - 1, 4)]["pair"]


# ---- Hessian -----------------------------------------------------------------------------------------------------------------------
HESSIAN_SIZES = [(1, 1), (1, 70), (4, 64), (5, 65), (130, 70)]


@pytest.mark.parametrize("sigma", [1.6, 12.8])
@pytest.mark.parametrize("h,w", HESSIAN_SIZES, ids=["%dx%d" % s for s in HESSIAN_SIZES])
def test_hessian_response_tile_edges(amd, h, w, sigma):
    """hessian_resp_kernel, 64 x 4 tiles: one pixel, one row, tile-exact, tile + 1 in both axes, many tiles; sigma^4 = 6.6 and 2.7e4."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    x = fc.blur_chain(fc.noise_image(h, w, 3 * h + w), 1.6)
    ctx = engine.utility_ctx(torch.device(DEV))
    xin = torch.from_numpy(x).to(DEV)
    out = torch.full((h, w), SENTINEL, dtype=torch.float32, device=DEV)
    check(lib.affnet_hessian_response(ctx, ptr(xin), ptr(out), h, w, np.float32(sigma ** 4), None), ctx, "hessian")
    torch.cuda.synchronize()
    want = fc.hessian_mirror(x, sigma)

    def where(i):
        edge = [n for n, hit in (("left", i[1] == 0), ("right", i[1] == w - 1), ("top", i[0] == 0), ("bottom", i[0] == h - 1)) if hit]
        return "tile column %d (lane %d), tile row %d (row %d of 4) in 64 x 4 tiles%s" % (
            i[1] // 64, i[1] % 64, i[0] // 4, i[0] % 4, "; neighbours clamped at the image's %s edge" % "/".join(edge) if edge else "")
    assert_exact("hessian %d x %d sigma %g" % (h, w, sigma), out.cpu().numpy(), want, where)
    if h > 1 and w > 1:
        assert want.max() > 0
    else:
        assert np.all(want == 0.0)                  # one row or one column: gyy (gxx) and gxy vanish exactly under replicate borders


# ---- detector at tile-edge image sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(65, 129), (127, 61)])
def test_detector_at_tile_edge_sizes(amd, h, w):
    """The fused hessian_nms_kernel (64 x 16 tiles, 2-px halo read from the blurred levels) at 4 x 16 + 1 rows / 2 x 64 + 1 columns and at
    8 x 16 - 1 rows / 64 - 3 columns: keys (octave, level, pixel) and responses equal the oracle's, the published pyramid equals the chain.
    All blurs here have >= 9 taps, where torch's CPU convolution is the chain on the hosts seen; should the oracle's own pyramid differ
    from the chain on the host that runs this test, that is printed as a finding about the reference host - the chain decides."""
    x = orc.synthetic_image(h, w, h + w)
    det = amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=60, border=5, num_Baum_iters=0).to(DEV)
    L, r = det(x.to(DEV))
    ex = orc.OracleExtractor(mrSize=5.192, num_features=60, border=5, num_Baum_iters=0)
    ex(x)
    ref = fc.pyramid_chain(x[0, 0].numpy(), 3, 1.6, 5)
    sizes, how = pyramid_launches(h, w, 1)
    assert len(det.scale_pyr) == len(ref) == len(ex.scale_pyr) == len(sizes) >= 3
    oracle_differs = []
    for o in range(len(ref)):
        for l in range(5):
            hw = how[(o, l)]
            got = det.scale_pyr[o][l].cpu().numpy()[0, 0]
            assert_exact("detector %d x %d pyramid octave %d level %d" % (h, w, o, l), got, ref[o][l],
                         lambda i: locate_blur(i[0], i[1], sizes[o][0], sizes[o][1], hw["k"], hw["bt_r"], True, hw["dec"]) if "decimated_from" not in hw else "decimated level")
            if not np.array_equal(ex.scale_pyr[o][l][0, 0].numpy(), ref[o][l]):
                oracle_differs.append((o, l))
    if oracle_differs:
        print("REFERENCE-HOST FINDING: torch's CPU pyramid on this host is not the fmaf chain at (octave, level) %s" % oracle_differs)
    record_parity("stage edges: detector %d x %d" % (h, w), oracle_pyramid_levels_not_the_chain=[list(v) for v in oracle_differs], rows=int(L.shape[0]))
    ids = det.last_ids.cpu().numpy().astype(np.int64)
    want = ex.detected
    want_ids = np.stack([want["oct"].numpy(), want["lev"].numpy(), want["pix"].numpy()], 1).astype(np.int64)
    note = " (the oracle's pyramid on this host differs from the chain at %s)" % oracle_differs if oracle_differs else ""
    assert 1 < len(want_ids) <= 60
    assert ids.shape == want_ids.shape and np.array_equal(ids, want_ids), "keys differ from the oracle%s: got %s ..., want %s ..." % (
        note, ids[:4].tolist(), want_ids[:4].tolist())
    assert np.array_equal(r.cpu().numpy(), want["resp"].numpy()), "responses differ from the oracle" + note
    assert len({int(v) for v in ids[:, 0]}) >= 2, "keypoints from one octave only: the small octaves are not exercised"


# ---- sampler -----------------------------------------------------------------------------------------------------------------------
SAMPLER_HW = (97, 131)
_c30, _s30 = np.cos(np.pi / 6), np.sin(np.pi / 6)
KINDS = [("isotropic", [[1.0, 0.0], [0.0, 1.0]]), ("rotated by 30 degrees", [[_c30, -_s30], [_s30, _c30]]), ("mirrored (det < 0)", [[1.0, 0.3], [0.2, -1.0]])]


def frame(theta, h, w):
    """Pixel-unit 2 x 3 frame -> the normalised float32 LAF the entry points take (LAF.py:407-429)."""
    t = np.asarray(theta, dtype=np.float64).reshape(2, 3)
    m = float(min(h, w))
    return (t / np.array([[m, m, w], [m, m, h]], dtype=np.float64)).astype(F32)


def box_of(laf, h, w, ps):
    """aff_tile_box on the frame exactly as grid_sample_kernel de-normalises it (fp32 products)."""
    m, fw, fh = F32(min(h, w)), F32(w), F32(h)
    return fc.tile_box(laf[0, 0] * m, laf[0, 1] * m, laf[0, 2] * fw, laf[1, 0] * m, laf[1, 1] * m, laf[1, 2] * fh, ps)


def gpu_sample(img, lafs, ps, n=None):
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    ctx = engine.utility_ctx(torch.device(DEV))
    h, w = img.shape
    lafs = np.asarray(lafs, dtype=F32).reshape(-1, 2, 3)
    n = lafs.shape[0] if n is None else n
    xin = torch.from_numpy(np.array(img, dtype=F32)).to(DEV)
    ld = torch.from_numpy(np.array(lafs, dtype=F32)).to(DEV)
    out = torch.full((lafs.shape[0], ps, ps), SENTINEL, dtype=torch.float32, device=DEV)
    check(lib.affnet_laf_grid_sample(ctx, ptr(xin), h, w, ptr(ld), n, ps, ptr(out), None), ctx, "laf_grid_sample")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def where_sample(lafs, h, w, ps):
    def where(i):
        x0, y0, tw, th, staged = box_of(lafs[i[0]], h, w, ps)
        return "patch %d row %d column %d; frame %s; box origin (%d, %d) size %d x %d = %d floats against min(4096, %d): %s" % (
            i[0], i[1], i[2], (lafs[i[0]] * np.array([[min(h, w)] * 2 + [w], [min(h, w)] * 2 + [h]])).round(3).tolist(), x0, y0, tw, th, tw * th, 2 * ps * ps,
            "staged in LDS" if staged else "direct gathers")
    return where


def boundary_frames(ps, h, w, centre=(65.3, 48.7)):
    """Per kind of frame: half-extents hx = (|t00| + |t01|) (ps - 1) / ps in half-pixel steps from 1.5 px below to 1 px above the first hx at
    which aff_tile_box stops staging (found by scanning box_of itself, so it moves with the source's formula)."""
    um = (ps - 1) / float(ps)
    lafs, kinds = [], []
    for name, M in KINDS:
        M = np.array(M)
        at = lambda hx: frame(np.hstack([M * (hx / (um * np.abs(M[0]).sum())), np.array(centre).reshape(2, 1)]), h, w)
        first_direct = next(hx for hx in np.arange(0.5, 100.0, 0.5) if not box_of(at(hx), h, w, ps)[4])
        for d in (-1.5, -1.0, -0.5, 0.0, 0.5, 1.0):
            if first_direct + d > 0:
                lafs.append(at(first_direct + d))
                kinds.append((name, first_direct + d))
    return np.stack(lafs), kinds


@pytest.fixture(scope="module")
def sampler_image():
    img = fc.noise_image(SAMPLER_HW[0], SAMPLER_HW[1], 77)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("ps", [19, 32, 41, 64])
def test_sampler_staged_direct_boundary(amd, sampler_image, ps):
    """Frames on both sides of tw * th <= min(4096, 2 ps^2): the LDS-staged box and the four predicated gathers must give the same bits.
    ps 19 / 32 / 41: the 2 ps^2 term decides (722, 2048, 3362); ps 64: the 4096-float LDS capacity does (2 * 64^2 = 8192)."""
    h, w = SAMPLER_HW
    lafs, kinds = boundary_frames(ps, h, w)
    boxes = [box_of(l, h, w, ps) for l in lafs]
    cap = min(4096, 2 * ps * ps)
    for name, _ in KINDS:
        sel = [b for b, k in zip(boxes, kinds) if k[0] == name]
        staged, direct = [b for b in sel if b[4]], [b for b in sel if not b[4]]
        assert len(staged) >= 2 and len(direct) >= 2, "%s frames at ps %d do not straddle the boundary: %s" % (name, ps, sel)
        assert all(b[2] * b[3] <= cap for b in staged) and all(b[2] * b[3] > cap for b in direct)
        assert max(b[2] * b[3] for b in staged) > 0.8 * cap                   # the largest staged box is close to the capacity
    if ps == 64:
        assert all(4096 < b[2] * b[3] <= 2 * ps * ps for b in boxes if not b[4]), "at ps 64 the LDS capacity, not 2 ps^2, must be what refuses"
    got = gpu_sample(sampler_image, lafs, ps)
    assert_exact("sampler boundary ps %d (%d frames)" % (ps, len(lafs)), got, fc.sample_mirror(sampler_image, lafs, ps), where_sample(lafs, h, w, ps))


def margin_frames(ps, h, w, per_side=3):
    """Staged frames whose taps reach the FIRST or LAST column / row of their box.  aff_tile_box adds one pixel on every side "for the fp32
    round trip of the coordinates"; for most frames (all of boundary_frames) no tap ever lands there, so a box that is one column short
    would go unnoticed.  The margin is used when cx + hx lies just below an integer (or cx - hx just above one): the sample coordinate,
    which goes through 2 g / size - 1 and back, then rounds across it.  Candidates are drawn with that property and kept where the
    mirror's own tap coordinates (sample_taps) do touch the box's edge."""
    rng = np.random.RandomState(1000 + ps)
    n = 3000
    um = (ps - 1) / float(ps)
    s, N, eps, side = rng.uniform(3.0, 9.0, n), rng.randint(20, 70, n), 10.0 ** rng.uniform(-7.0, -4.3, n), rng.randint(0, 4, n)
    near = np.where(side % 2 == 0, N - eps - s * um + 0.5, N + eps + s * um + 0.5)              # far edge just below N / near edge just above N
    cx, cy = np.where(side < 2, near, 60.3), np.where(side < 2, 48.7, near)
    lafs = np.stack([frame([[s[i], 0.0, cx[i]], [0.0, s[i], cy[i]]], h, w) for i in range(n)])
    x0, y0 = fc.sample_taps(h, w, lafs, ps)[:2]
    picked = {"right": [], "left": [], "bottom": [], "top": []}
    for i in range(n):
        bx, by, tw, th, staged = box_of(lafs[i], h, w, ps)
        if not staged:
            continue
        hit = {"right": x0[i].max() + 1 == bx + tw - 1, "left": x0[i].min() == bx, "bottom": y0[i].max() + 1 == by + th - 1, "top": y0[i].min() == by}
        for k, v in hit.items():
            if v and len(picked[k]) < per_side:
                picked[k].append(i)
    return lafs, picked


@pytest.mark.parametrize("ps", [19, 32])
def test_sampler_taps_in_the_margin_of_the_staged_box(amd, sampler_image, ps):
    h, w = SAMPLER_HW
    lafs, picked = margin_frames(ps, h, w)
    assert all(len(v) >= 2 for v in picked.values()), "no staged frame found whose taps reach the box's %s margin" % [k for k, v in picked.items() if len(v) < 2]
    sel = lafs[sorted({i for v in picked.values() for i in v})]
    got = gpu_sample(sampler_image, sel, ps)
    assert_exact("sampler margin taps ps %d (%d frames)" % (ps, len(sel)), got, fc.sample_mirror(sampler_image, sel, ps), where_sample(sel, h, w, ps))


@pytest.mark.parametrize("ps", [1, 2])
def test_sampler_patch_sizes_that_are_never_staged(amd, sampler_image, ps):
    """The smallest box is 4 x 4 = 16 floats (1-px margins), more than 2 ps^2 for ps = 1 and 2: every frame takes the direct gathers."""
    h, w = SAMPLER_HW
    assert 16 > 2 * ps * ps
    lafs = np.stack([frame(np.hstack([np.array(M) * s, [[cx], [cy]]]), h, w) for (_, M) in KINDS for s in (0.01, 0.7, 3.0, 11.0)
                     for (cx, cy) in ((65.3, 48.7), (0.2, 96.9))])
    assert not any(box_of(l, h, w, ps)[4] for l in lafs)
    got = gpu_sample(sampler_image, lafs, ps)
    assert_exact("sampler ps %d (%d frames, all direct)" % (ps, len(lafs)), got, fc.sample_mirror(sampler_image, lafs, ps), where_sample(lafs, h, w, ps))


@pytest.mark.parametrize("ps", [2, 19, 32, 41])
def test_sampler_borders(amd, sampler_image, ps):
    """Boxes with a negative origin in x, in y and in both; frames hanging over the right and bottom edge; frames wholly outside (all zeros,
    staged boxes that hold nothing but padding); a frame with hx >= 4096 (rejected by aff_tile_box before the box is computed); n = 0."""
    h, w = SAMPLER_HW
    A = np.array([[6.0, 1.0], [-1.5, 5.0]])
    centres = [(1.5, 40.0), (60.0, 1.2), (0.7, 0.4), (129.6, 95.9), (-80.0, -80.0), (300.0, 50.0), (60.0, -40.0)]
    lafs = [frame(np.hstack([A, [[cx], [cy]]]), h, w) for cx, cy in centres]
    lafs.append(frame([[5000.0, 0.0, 65.5], [0.0, 3.0, 48.5]], h, w))
    lafs = np.stack(lafs)
    boxes = [box_of(l, h, w, ps) for l in lafs]
    if ps >= 19:
        assert all(b[4] for b in boxes[:7]), boxes
        assert boxes[0][0] < 0 <= boxes[0][1] and boxes[1][1] < 0 <= boxes[1][0] and boxes[2][0] < 0 and boxes[2][1] < 0
        assert boxes[3][0] + boxes[3][2] > w and boxes[3][1] + boxes[3][3] > h
        assert boxes[4][0] + boxes[4][2] < 0 and boxes[5][0] >= w and boxes[6][1] + boxes[6][3] < 0
    assert not boxes[7][4] and (ps < 19 or boxes[7] == (0, 0, 0, 0, False))             # 5000 * (ps - 1) / ps >= 4096 from ps = 6 on
    want = fc.sample_mirror(sampler_image, lafs, ps)
    assert np.all(want[4:7] == 0.0) and np.abs(want[:4]).max() > 1.0
    assert (want[7] == 0.0).mean() >= 0.5 and (ps % 2 == 0 or np.abs(want[7]).max() > 0.0)          # mostly outside; the centre column of an odd ps is inside
    got = gpu_sample(sampler_image, lafs, ps)
    assert_exact("sampler borders ps %d" % ps, got, want, where_sample(lafs, h, w, ps))
    untouched = gpu_sample(sampler_image, lafs, ps, n=0)
    assert np.all(untouched == F32(SENTINEL)), "n = 0 wrote to the output"


@pytest.mark.parametrize("ps", [19, 32])
def test_sampler_pyramid_entry_point_batch_counts_and_id_clamping(amd, ps):
    """affnet_pyr_grid_sample on a batch of two 64 x 80 images (octaves 64 x 80, 32 x 40, 16 x 20): ids over every (octave, level) plus ids
    out of range on both sides of both fields (clamped by the kernel, and the same way here); per-image counts, one of them above n_max;
    rows at or beyond an image's count keep what the output held.  The levels are read back from the device and handed to the mirror,
    so the sampler is compared on its own."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    h, w = 64, 80
    ctx, level, _ = build_pyramids(h, w, [11, 12])
    sizes, n_lev = list(ctx.plan.sizes), ctx.plan.levels_per_octave
    assert sizes == [(64, 80), (32, 40), (16, 20)] and n_lev == 5
    pairs = [(o, l) for o in range(3) for l in range(5)] + [(-1, 2), (3, 1), (1, -3), (0, 9), (-7, -7), (99, 99)]
    n_max = len(pairs)
    rng = np.random.RandomState(ps)
    lafs = np.zeros((2, n_max, 2, 3), dtype=F32)
    for b in range(2):
        for i in range(n_max):
            a, s = rng.uniform(0, 2 * np.pi), rng.uniform(0.08, 0.45)
            lafs[b, i, :, :2] = s * np.array([[np.cos(a), -np.sin(a) * 0.7], [np.sin(a), np.cos(a) * 1.3]])
            lafs[b, i, :, 2] = rng.uniform(-0.05, 1.05, 2)
    ids = np.zeros((2, n_max, 3), dtype=np.int32)
    ids[:, :, :2] = np.array(pairs, dtype=np.int32)[None]
    ids[:, :, 2] = 123456                                              # the pixel field is not read by the sampler
    dev = torch.device(DEV)
    ld, idd = torch.from_numpy(lafs).to(dev), torch.from_numpy(ids).to(dev)
    want = np.zeros((2, n_max, ps, ps), dtype=F32)
    for b in range(2):
        for i, (o, l) in enumerate(pairs):
            o, l = min(max(o, 0), 2), min(max(l, 0), 4)
            want[b, i] = fc.sample_mirror(level(b, o, l), lafs[b, i:i + 1], ps)[0]
    assert np.abs(want).max() > 1.0 and not np.array_equal(want[0], want[1])
    for counts in ([n_max, 3], [0, n_max], [n_max + 7, 1], None):
        out = torch.full((2, n_max, ps, ps), SENTINEL, dtype=torch.float32, device=dev)
        cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=dev)
        check(lib.affnet_pyr_grid_sample(ctx.handle, ptr(ld), ptr(idd), ptr(cnt), n_max, ps, ptr(out), engine.stream_of(dev)), ctx.handle, "pyr_grid_sample")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        expect = want.copy()
        for b in range(2):
            expect[b, (n_max if counts is None else min(counts[b], n_max)):] = F32(SENTINEL)
        assert_exact("pyramid sampler ps %d counts %s" % (ps, counts), got, expect,
                     lambda i: "image %d row %d -> ids (octave %d, level %d); patch row %d column %d" % (i[0], i[1], pairs[i[1]][0], pairs[i[1]][1], i[2], i[3]))
