"""CPU: pins of the plain fp32 references in tests/_fp32_chain.py.  tests/test_gpu_stage_edges.py compares the HIP blur, Hessian and
sampler kernels with these mirrors EXACTLY, so a wrong mirror would make every one of those tests meaningless; each mirror is tied
here to something the project already trusts:

  fma32           libm fmaf (ctypes), on random triples and on constructed fp32 half-way cases
  blur_chain      oracle gaussian_blur (torch CPU conv2d) on inputs of more than 20480 elements, where ATen runs oneDNN
  pyramid_chain   the committed digests of the unmodified reference's pyramid (tests/golden/synth_240x320_s1_n300.npz)
  hessian_mirror  oracle hessian_response
  sample_mirror   tests/golden/sampler_synth.npz (unmodified reference, authoring host), the library's host base grid
"""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest
import torch

import affnet_oracle as orc
import _fp32_chain as fc

from _fp32_chain import noise_image as _np_image, sigma_for_taps

F32 = np.float32


# ---- fma32 ---------------------------------------------------------------------------------------------------------------------------
def _fma_inputs():
    rng = np.random.RandomState(11)
    n = 20000
    # random triples over a wide exponent range, c of comparable or unrelated magnitude
    a = (rng.standard_normal(n) * 2.0 ** rng.randint(-20, 20, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.randint(-20, 20, n)).astype(F32)
    c = np.where(rng.rand(n) < 0.5, -(a.astype(np.float64) * b) * (1.0 + rng.standard_normal(n) * 1e-3), rng.standard_normal(n) * 2.0 ** rng.randint(-30, 30, n)).astype(F32)
    sets = [(a, b, c)]
    # family 1: a * b is an odd 25-bit integer 2 N + 1 scaled by a power of two - exactly half way between two fp32 values - and c is tiny,
    # of either sign: the fma must round AWAY from the tie on the side of c, the float64 sum is the tie itself
    pa = rng.randint(1 << 12, 1 << 13, n) | 1                      # 13-bit odd
    pb = rng.randint(1 << 11, 1 << 12, n) | 1                      # 12-bit odd
    keep = (pa * pb >= (1 << 24)) & (pa * pb < (1 << 25))
    pa, pb = pa[keep], pb[keep]
    m = len(pa)
    sa, sb = 2.0 ** rng.randint(-12, 12, m), 2.0 ** rng.randint(-12, 12, m)
    sign = rng.choice([-1.0, 1.0], m)
    a1, b1 = (pa * sa * sign).astype(F32), (pb * sb).astype(F32)
    c1 = (rng.choice([-1.0, 1.0], m) * sa * sb * 2.0 ** rng.randint(-60, -32, m)).astype(F32)
    sets.append((a1, b1, c1))
    # family 2: c = +- integer N in (2^23, 2^24) (fp32 ulp 1) and a * b = +- 0.5 (1 - 2^-46), signs independent: |c + a b| lies 2^-47
    # below the tie N + 0.5 (same signs) or above the tie N - 0.5 (opposite signs); the float64 sum (ulp 2^-29 there) is the tie itself
    N = rng.randint((1 << 23) + 2, 1 << 24, n).astype(np.float64)
    a2 = ((1.0 + 2.0 ** -23) * rng.choice([-1.0, 1.0], n)).astype(F32)
    b2 = np.full(n, 0.5 * (1.0 - 2.0 ** -23)).astype(F32)
    sets.append((a2, b2, (N * rng.choice([-1.0, 1.0], n)).astype(F32)))
    return tuple(np.concatenate([s[i] for s in sets]) for i in range(3))


def test_fma32_equals_libm_fmaf_where_the_double_rounding_form_does_not():
    """Zero mismatches against libm's fmaf (nothing preloaded; the function is called value by value through ctypes).  The same inputs
    make (a64 * b64 + c64).astype(f32) disagree with fmaf: the half-way cases are really in the set."""
    path = ctypes.util.find_library("m")
    assert path, "libm not found"
    libm = ctypes.CDLL(path)
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    a, b, c = _fma_inputs()
    want = np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=F32)
    assert np.isfinite(want).all()
    got = fc.fma32(a, b, c)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "fma32 != fmaf at %d of %d triples, first (a, b, c) = %r: got %r, want %r" % (
        bad.size, a.size, (a[bad[0]], b[bad[0]], c[bad[0]]), got[bad[0]], want[bad[0]])
    naive_wrong = int((fc.naive_fma32(a, b, c).view(np.uint32) != want.view(np.uint32)).sum())
    print("fma32: 0 of %d triples differ from fmaf; the double-rounding form differs at %d" % (a.size, naive_wrong))
    assert naive_wrong >= 1, "the constructed ties do not exercise the double rounding"
    # scalars and broadcasting
    assert fc.fma32(F32(3.0), F32(0.5), F32(1.0)) == F32(2.5) and fc.fma32(F32(2.0), np.ones((2, 3), F32), F32(1.0)).shape == (2, 3)
    assert np.array_equal(fc.fma32(np.zeros(3, F32), F32(5.0), F32(-0.0)), np.zeros(3, F32))


# ---- blur ----------------------------------------------------------------------------------------------------------------------------
def test_taps_equal_the_oracle_and_the_host_plan():
    from affnet_amd.host_plan import gaussian_taps
    for k in range(1, 41, 2):
        s = sigma_for_taps(k)
        t = fc.gaussian_taps(s)
        assert t.shape == (k, k)
        assert np.array_equal(t, orc.gauss_kernel_2d(s)[0]) and np.array_equal(t, gaussian_taps(s))
    for (h, w, nl, s0, b) in [(240, 320, 3, 1.6, 5), (193, 257, 3, 1.6, 5), (256, 256, 1, 1.6, 5), (65, 129, 3, 1.6, 5), (240, 320, 2, 0.5, 5), (127, 61, 4, 1.6, 0)]:
        first, octs = fc.pyramid_plan(h, w, nl, s0, b)
        ref = orc.pyramid_plan(h, w, nl, s0, b)
        assert first == ref["first_blur"]
        assert [(o[0], o[1]) for o in octs] == [(o["h"], o["w"]) for o in ref["octaves"]]
        assert [o[2] for o in octs] == [o["blur_sigmas"] for o in ref["octaves"]]


@pytest.mark.parametrize("k,h,w", [(3, 130, 200), (9, 130, 200), (15, 130, 200), (25, 130, 200), (37, 130, 200), (3, 240, 320), (15, 240, 320), (37, 240, 320)])
def test_blur_chain_equals_the_oracle_on_large_inputs(k, h, w):
    """More than 20480 elements: ATen's CPU conv2d runs oneDNN, whose direct convolution IS the row-major fmaf chain per pixel."""
    assert h * w > 20480
    x = _np_image(h, w, k)
    s = sigma_for_taps(k)
    want = orc.gaussian_blur(torch.from_numpy(x).view(1, 1, h, w), s)[0, 0].numpy()
    got = fc.blur_chain(x, s)
    d = np.abs(got.astype(np.float64) - want)
    assert np.array_equal(got, want), "k = %d, %d x %d: %d pixels differ, max %g" % (k, h, w, int((d > 0).sum()), d.max())


def test_blur_chain_is_the_specification_on_small_inputs_whatever_torch_does():
    """The specification csrc/pyramid.hip implements is the row-major fmaf chain from 0 (its header comment), which is what
    blur_chain computes and what torch's conv2d computes wherever it runs oneDNN.  For 3 x 3 kernels on inputs of <= 20480 elements ATen
    takes im2col + MKL sgemm instead, whose summation order is MKL's own: on some CPUs it equals the chain, on others ~45 % of the pixels
    differ by up to 2 ulp.  That is a property of the host, so nothing is asserted about it; what IS asserted: the chain does not depend on
    the input size (the small image embedded in a large edge-padded one, which torch blurs with oneDNN, gives the same pixels), and torch's
    small-input result is a correct 9-term sum: two evaluations of 9 products of values <= 255 with weights that add up to 1 make at most
    9 roundings of <= half an ulp of 255 each, so they differ by at most 9 ulp whatever the order."""
    h, w = 40, 56
    assert h * w <= 20480
    x = _np_image(h, w, 5)
    s = sigma_for_taps(3)
    got = fc.blur_chain(x, s)
    big = np.pad(x, ((0, 160), (0, 144)), mode="edge")              # 200 x 200: the same replicate neighbourhood for the rows / columns above
    assert big.size > 20480
    ref = orc.gaussian_blur(torch.from_numpy(big).view(1, 1, 200, 200), s)[0, 0].numpy()[:h, :w]
    assert np.array_equal(got, ref), "the chain on a small input differs from the oneDNN path on the same pixels"
    small = orc.gaussian_blur(torch.from_numpy(x).view(1, 1, h, w), s)[0, 0].numpy()
    d = np.abs(got.astype(np.float64) - small)
    print("K = 3 on %d x %d: torch's small-input path differs from the chain at %d of %d pixels, max %.3g" % (h, w, int((d > 0).sum()), d.size, d.max()))
    assert d.max() <= 9 * np.spacing(F32(255.0))


def test_pyramid_chain_reproduces_the_reference_digests(golden_dir):
    """pyr_samples / pyr_sums of tests/golden/synth_240x320_s1_n300.npz come from the unmodified reference; computed as
    tests/test_gpu_parity.py::test_pyramid_and_detector_exact computes them from the HIP pyramid."""
    g = np.load(os.path.join(golden_dir, "synth_240x320_s1_n300.npz"))
    x = orc.synthetic_image(240, 320, 1)[0, 0].numpy()
    pyr = fc.pyramid_chain(x, 3, 1.6, 5)
    sums, k = [], 0
    for o in range(len(pyr)):
        assert len(pyr[o]) == 5
        for l in range(5):
            flat = pyr[o][l].reshape(-1)
            assert np.array_equal(flat[np.linspace(0, flat.size - 1, 16).astype(np.int64)], g["pyr_samples"][k]), (o, l)
            sums.append(pyr[o][l].astype(np.float64).sum())
            k += 1
    assert k == len(g["pyr_samples"])
    assert np.array_equal(np.array(sums), g["pyr_sums"])


# ---- Hessian -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,sigma", [(130, 200, 2.0158736798317967), (240, 320, 1.6), (150, 137, 3.2)])
def test_hessian_mirror_equals_the_oracle(h, w, sigma):
    assert h * w > 20480
    x = orc.gaussian_blur(torch.from_numpy(_np_image(h, w, h)).view(1, 1, h, w), 1.6)
    want = orc.hessian_response(x, sigma)[0, 0].numpy()
    got = fc.hessian_mirror(x[0, 0].numpy(), sigma)
    assert np.array_equal(got, want), "%d pixels differ, max %g" % (int((got != want).sum()), np.abs(got - want).max())
    assert got.max() > 0


# ---- sampler -------------------------------------------------------------------------------------------------------------------------
def test_sample_mirror_reproduces_the_reference_patches(golden_dir):
    g = np.load(os.path.join(golden_dir, "sampler_synth.npz"))
    x = orc.synthetic_image(240, 320, 1)[0, 0].numpy()
    for ps, key in [(32, "p32"), (41, "p41")]:
        want = g[key].reshape(-1, ps, ps)
        got = fc.sample_mirror(x, g["lafs"], ps)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "ps %d: %d of %d elements differ, max %g" % (ps, int((got != want).sum()), want.size, np.abs(got - want).max())


def test_base_grid_equals_the_library_and_torch():
    for ps in range(2, 65):
        assert np.array_equal(fc.base_grid(ps), (torch.linspace(-1, 1, ps) * (ps - 1) / ps).numpy()), ps
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "affnet_amd", "libaffnet_hip.so")
    if not os.path.isfile(so):
        pytest.skip("libaffnet_hip.so is not built: affnet_host_base_grid not compared")
    lib = ctypes.CDLL(so)
    lib.affnet_host_base_grid.restype = ctypes.c_int
    lib.affnet_host_base_grid.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    for ps in range(1, 65):
        buf = (ctypes.c_float * ps)()
        assert lib.affnet_host_base_grid(ps, buf) == 0
        assert np.array_equal(np.array(list(buf), dtype=F32), fc.base_grid(ps)), ps


def test_tile_box_restatement_matches_the_source():
    """tile_box decides in tests/test_gpu_stage_edges.py which sampler path a frame takes; its constants are the ones in the source."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = open(os.path.join(root, "affnet_amd", "csrc", "common.h")).read()
    laf = open(os.path.join(root, "affnet_amd", "csrc", "laf_ops.hip")).read()
    for frag in ("if (tw * th > cap || tw * th > 2 * ps * ps) return t;", "(int)floorf(cx - hx) - 1, x1 = (int)floorf(cx + hx) + 2;",
                 "(int)floorf(cy - hy) - 1, y1 = (int)floorf(cy + hy) + 2;", "hx < 4096.0f && hy < 4096.0f", "const float cx = t02 - 0.5f, cy = t12 - 0.5f;"):
        assert frag in common, frag
    assert "#define GS_TILE_CAP 4096" in laf
    # |t00| + |t01| = 20 at (50.5, 40.5), ps 32: hx = 20 * 31 / 32 = 19.375 -> columns 29 .. 71, rows 19 .. 61
    assert fc.tile_box(10.0, 10.0, 50.5, 10.0, 10.0, 40.5, 32) == (29, 19, 43, 43, True)
    assert fc.tile_box(12.0, 12.0, 50.5, 12.0, 12.0, 40.5, 32)[4] is False            # 50 x 50 > 2 * 32 * 32
    assert fc.tile_box(5000.0, 0.0, 50.5, 1.0, 1.0, 40.5, 32) == (0, 0, 0, 0, False)


def test_stage_edge_dispatch_restatement_and_size_coverage():
    """tests/test_gpu_stage_edges.py restates the dispatch arithmetic of csrc/pyramid.hip to say which tile shape, store path and launch
    each of its cases reaches; the constants it restates are the ones in the source, and its pyramid sizes cover what it says they cover:
    the levels whose blur also writes the next octave (every octave but the last) have a last row / column that is decimated (odd size)
    and one that is not (even size), in both axes independently, on the float4 + packed path (w % 4 == 0) and on the scalar one."""
    from test_gpu_stage_edges import PAIR_SIZES, blur_bt_r, pair_bt_r, pyramid_launches
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "affnet_amd", "csrc", "pyramid.hip")).read()
    for frag in ("#define BT_X 64", "const int tiles64 = aff_cdiv(w, BT_X) * aff_cdiv(h, 64) * batch;", "if (tiles64 >= 1024) {",
                 "const int t64 = (aff_cdiv(wa, BT_X) * aff_cdiv(ha, 64) + aff_cdiv(wb, BT_X) * aff_cdiv(hb, 64)) * batch;", "const int ty = t64 >= 1024 ? 64 : 16;",
                 "if (ka != 15 || kb != 9) return false;", "if (x + 3 < w && (w & 3) == 0 && ((size_t)out & 15) == 0) {", "const int dec_level = L - 2;"):
        assert frag in src, frag
    assert blur_bt_r(193, 257, 52) == 4 and blur_bt_r(193, 257, 51) == 1 and blur_bt_r(256, 256, 64) == 4 and blur_bt_r(256, 256, 63) == 1
    assert pair_bt_r(193, 257, 97, 129, 52) == 4 and blur_bt_r(97, 129, 52) == 1
    decimated = [s for h, w in PAIR_SIZES for s in pyramid_launches(h, w, 1)[0][:-1]]
    assert {(h % 2, w % 2) for h, w in decimated} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(w % 4 == 0, h % 2) for h, w in decimated} >= {(True, 0), (True, 1), (False, 0), (False, 1)}
    sizes, how = pyramid_launches(240, 320, 1)
    assert [how[(0, l)]["k"] for l in range(5)] == [11, 9, 11, 13, 15] and how[(0, 4)]["pair"] and how[(1, 1)]["pair"] and how[(0, 3)]["dec"]
