"""Plain numpy references of the three detector-side stages, written as the fp32 operation sequences the HIP kernels claim to replay
(csrc/pyramid.hip header, hessian_resp_kernel in csrc/detect.hip, the comment above aff_sample_bilinear in csrc/common.h).  numpy only:
no torch, no affnet_amd, no GPU - so the result does not depend on which convolution path a CPU library picks on the host that runs
the test (torch's CPU conv2d is NOT the row-major fmaf chain for 3 x 3 kernels on inputs of <= 20480 elements: ATen leaves oneDNN for
im2col + MKL sgemm there).  tests/test_fp32_chain_host.py ties every function of this file to something the project already trusts
(libm fmaf, the oracle on large inputs, the golden digests of the unmodified reference).

fp32 fused multiply-add on arrays: the product of two fp32 values is exact in float64 (48 <= 53 bits); the float64 sum p + c is not,
and rounding it to fp32 afterwards rounds twice - wrong whenever the float64 sum lands exactly on an fp32 half-way point.  fma32 takes
the TwoSum error of p + c and, where the sum was inexact and its last float64 mantissa bit is even, moves it one float64 ulp towards
the error (round to odd); 53 >= 24 + 2 bits then makes the final rounding to fp32 the correctly rounded fma."""
import numpy as np

F32 = np.float32


def _round_odd_sum(p, c):
    """float64 arrays p, c -> p + c rounded to odd (float64).  p + c must not overflow; zeros, subnormal fp32 inputs and exact sums pass
    through unchanged."""
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                        # TwoSum: s + e == p + c exactly
    fix = (e != 0.0) & ((s.view(np.int64) & 1) == 0)
    if fix.any():
        idx = np.flatnonzero(fix)
        sf = s.reshape(-1)
        sf[idx] = np.nextafter(sf[idx], np.where(e.reshape(-1)[idx] > 0.0, np.inf, -np.inf))
    return s


def fma32(a, b, c):
    """Correctly rounded fp32 fma(a, b, c) = round32(a * b + c), element-wise with numpy broadcasting."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    p, c64 = np.broadcast_arrays(a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64))
    return _round_odd_sum(np.array(p), np.array(c64)).astype(F32)


def naive_fma32(a, b, c):
    """The double-rounding form (a64 * b64 + c64).astype(f32): kept to show, in the host test, that fma32's inputs contain its failures."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def noise_image(h, w, seed):
    """(h, w) float32 image, 0 .. 255: white noise + 4 x 4 block noise + a sine, from numpy's seeded generator alone (the same bits on
    every host; oracle synthetic_image needs >= 4 px per side and goes through torch's interpolation)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    blocks = rng.rand(-(-h // 4), -(-w // 4)).repeat(4, 0).repeat(4, 1)[:h, :w]
    return (96.0 * rng.rand(h, w) + 40.0 * (1.0 + np.sin(0.37 * xx + 0.11 * yy + seed)) + 79.0 * blocks).astype(F32)


# ---- Gaussian blur and pyramid -----------------------------------------------------------------------------------------------------
def sigma_for_taps(k):
    """A sigma whose Gaussian has k x k taps: int(6 sigma + 1) | 1 == k."""
    s = (k - 0.5) / 6.0
    assert (int(6.0 * s + 1.0) | 1) == k
    return s


def gaussian_taps(sigma):
    """(k, k) float32 taps, k = int(6 sigma + 1) | 1, sampled at linspace(-k/2, k/2, k) and sum-normalised in float64: the formula of
    oracle/affnet_oracle.py gauss_kernel_2d and affnet_amd/host_plan.py gaussian_taps (equality checked in the host test)."""
    k = int(2.0 * 3.0 * sigma + 1.0)
    k += (k % 2 == 0)
    half = k / 2
    ax = np.linspace(-half, half, k)
    xv, yv = np.meshgrid(ax, ax, sparse=False, indexing="xy")
    ker = np.exp(-((xv ** 2 + yv ** 2) / (2.0 * sigma * sigma)))
    ker /= np.sum(ker)
    return ker.astype(F32)


def blur_chain_taps(img, taps):
    """Replicate padding by k // 2, then per output pixel ONE fmaf chain from 0 over the k x k taps in row-major order."""
    img = np.ascontiguousarray(img, dtype=F32)
    taps = np.asarray(taps, dtype=F32)
    assert img.ndim == 2 and taps.ndim == 2 and taps.shape[0] == taps.shape[1] and taps.shape[0] % 2 == 1
    k = taps.shape[0]
    h, w = img.shape
    xp = np.pad(img, k // 2, mode="edge").astype(np.float64)
    t64 = taps.astype(np.float64)
    acc = np.zeros((h, w), dtype=np.float64)             # always holds fp32 values
    for i in range(k):
        for j in range(k):
            acc = _round_odd_sum(xp[i:i + h, j:j + w] * t64[i, j], acc).astype(F32).astype(np.float64)
    return acc.astype(F32)


def blur_chain(img, sigma):
    return blur_chain_taps(img, gaussian_taps(sigma))


def pyramid_plan(height, width, n_levels=3, init_sigma=1.6, border=5):
    """(first blur sigma or None, [(h, w, [blur sigma of level 1 .. n_levels + 1])] per octave): the loop and stop rule of
    oracle/affnet_oracle.py pyramid_plan."""
    step = 2 ** (1.0 / float(n_levels))
    min_size = 2 * border + 2 + 1
    cur, first = 0.5, None
    if init_sigma > cur:
        first = float(np.sqrt(init_sigma ** 2 - cur ** 2))
        cur = init_sigma
    h, w, octaves = int(height), int(width), []
    while True:
        blur = []
        for _ in range(1, n_levels + 2):
            blur.append(float(cur * np.sqrt(step * step - 1.0)))
            cur *= step
        octaves.append((h, w, blur))
        nh, nw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        cur = init_sigma
        if nh <= min_size or nw <= min_size:
            break
        h, w = nh, nw
    return first, octaves


def pyramid_chain(img, n_levels=3, init_sigma=1.6, border=5):
    """pyr[o][l] as 2-D float32 arrays: oracle/affnet_oracle.py scale_pyramid with blur_chain as the blur and [::2, ::2] as
    avg_pool2d(kernel 1, stride 2) of level n_levels."""
    img = np.ascontiguousarray(img, dtype=F32)
    first, octaves = pyramid_plan(img.shape[0], img.shape[1], n_levels, init_sigma, border)
    cur = blur_chain(img, first) if first is not None else img
    pyr = []
    for (h, w, blurs) in octaves:
        assert cur.shape == (h, w)
        levels, nxt = [cur], None
        for i, bs in enumerate(blurs, start=1):
            cur = blur_chain(cur, bs)
            levels.append(cur)
            if i == n_levels:
                nxt = np.ascontiguousarray(cur[::2, ::2])
        pyr.append(levels)
        cur = nxt
    return pyr


# ---- Hessian response --------------------------------------------------------------------------------------------------------------
def hessian_mirror(img, sigma):
    """|gxx gyy - gxy^2| sigma^4 with replicate borders, every operation a separately rounded fp32 operation in the order of
    hessian_resp_kernel: (l - 2c) + r, 0.5 a - 0.5 b twice; the factor arrives the way the callers pass it, np.float32(sigma ** 4)."""
    x = np.ascontiguousarray(img, dtype=F32)
    h, w = x.shape
    xm, xp = np.maximum(np.arange(w) - 1, 0), np.minimum(np.arange(w) + 1, w - 1)
    ym, yp = np.maximum(np.arange(h) - 1, 0), np.minimum(np.arange(h) + 1, h - 1)
    two, half = F32(2.0), F32(0.5)
    gxx = (x[:, xm] - two * x) + x[:, xp]
    gyy = (x[ym, :] - two * x) + x[yp, :]
    gu = half * x[ym][:, xm] - half * x[ym][:, xp]
    gd = half * x[yp][:, xm] - half * x[yp][:, xp]
    gxy = half * gu - half * gd
    out = np.abs(gxx * gyy - gxy * gxy) * F32(sigma ** 4)
    assert out.dtype == F32
    return out


# ---- patch sampler -----------------------------------------------------------------------------------------------------------------
def base_grid(ps):
    """(linspace(-1, 1, ps) * (ps - 1)) / ps as torch computes it on the CPU: element i = fma(step, i, -1) below ps // 2 and
    fma(-step, ps - 1 - i, 1) from there on (csrc/context.hip aff_base_grid)."""
    if ps == 1:
        return np.zeros(1, dtype=F32)
    step = F32(2.0) / F32(ps - 1)
    i = np.arange(ps)
    lo = fma32(step, i.astype(F32), F32(-1.0))
    hi = fma32(-step, (ps - 1 - i).astype(F32), F32(1.0))
    v = np.where(i < ps // 2, lo, hi).astype(F32)
    return (v * F32(ps - 1)) / F32(ps)


def sample_taps(h, w, lafs, ps):
    """The sampler's coordinate arithmetic for an h x w image: (x0, y0, nw, ne, sw, se) per sample, each (n, ps, ps) - column / row of
    the north-west tap (int64, after the kernel's clamp to [-2, size + 1]) and the four bilinear weights (float32):
    theta = LAF * [[m, m, w], [m, m, h]];  g = fma(1, t02, fma(v, t01, u * t00));  gn = 2 g / size - 1;  i = fma(gn + 1, size / 2, -0.5)."""
    lafs = np.asarray(lafs, dtype=F32).reshape(-1, 2, 3)
    n = lafs.shape[0]
    fw, fh, m = F32(w), F32(h), F32(min(h, w))
    t = lambda r, c, s: (lafs[:, r, c] * s).astype(F32).reshape(n, 1, 1)
    t00, t01, t02 = t(0, 0, m), t(0, 1, m), t(0, 2, fw)
    t10, t11, t12 = t(1, 0, m), t(1, 1, m), t(1, 2, fh)
    bg = base_grid(ps)
    u = np.broadcast_to(bg.reshape(1, 1, ps), (n, ps, ps))           # column coordinate
    v = np.broadcast_to(bg.reshape(1, ps, 1), (n, ps, ps))           # row coordinate
    one, two, half = F32(1.0), F32(2.0), F32(0.5)
    gx = fma32(one, t02, fma32(v, t01, u * t00))
    gy = fma32(one, t12, fma32(v, t11, u * t10))
    gx = two * gx / fw - one
    gy = two * gy / fh - one
    ix = fma32(gx + one, fw * half, F32(-0.5))
    iy = fma32(gy + one, fh * half, F32(-0.5))
    x0f, y0f = np.floor(ix), np.floor(iy)
    x1f, y1f = x0f + one, y0f + one
    wx1, wx0, wy1, wy0 = ix - x0f, x1f - ix, iy - y0f, y1f - iy
    nw, ne, sw, se = wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1
    x0 = np.minimum(np.maximum(x0f, F32(-2.0)), fw + one).astype(np.int64)
    y0 = np.minimum(np.maximum(y0f, F32(-2.0)), fh + one).astype(np.int64)
    for a in (gx, ix, nw, se):
        assert a.dtype == F32
    return x0, y0, nw, ne, sw, se


def sample_mirror(img, lafs, ps):
    """(n, ps, ps) float32 patches of the 2-D image `img` along the NORMALISED frames `lafs` (n, 2, 3): LAF.py:313-324 + affine_grid +
    grid_sample (bilinear, zero padding, align_corners = False) in the fp32 sequence documented above aff_sample_bilinear: the
    coordinates and weights of sample_taps, zero padding, out = fma(vse, se, fma(vsw, sw, fma(vne, ne, vnw * nw)))."""
    img = np.ascontiguousarray(img, dtype=F32)
    h, w = img.shape
    x0, y0, nw, ne, sw, se = sample_taps(h, w, lafs, ps)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(inside, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], F32(0.0)).astype(F32)

    out = fma32(tap(y0 + 1, x0 + 1), se, fma32(tap(y0 + 1, x0), sw, fma32(tap(y0, x0 + 1), ne, tap(y0, x0) * nw)))
    assert out.dtype == F32
    return out


def tile_box(t00, t01, t02, t10, t11, t12, ps, cap=4096):
    """csrc/common.h aff_tile_box restated: (x0, y0, tw, th, staged) of the LDS box of one patch from its de-normalised frame (fp32
    scalars).  staged is False where the kernel takes the four predicated gathers; tw, th are then what the box WOULD have been (or 0
    where the kernel rejects the frame before computing it)."""
    t00, t01, t02, t10, t11, t12 = (F32(v) for v in (t00, t01, t02, t10, t11, t12))
    um = F32(ps - 1) / F32(ps)
    hx = (np.abs(t00) + np.abs(t01)) * um
    hy = (np.abs(t10) + np.abs(t11)) * um
    cx, cy = t02 - F32(0.5), t12 - F32(0.5)
    if not (hx < F32(4096.0) and hy < F32(4096.0) and abs(cx) < F32(1.0e6) and abs(cy) < F32(1.0e6)):
        return 0, 0, 0, 0, False
    x0, x1 = int(np.floor(cx - hx)) - 1, int(np.floor(cx + hx)) + 2
    y0, y1 = int(np.floor(cy - hy)) - 1, int(np.floor(cy + hy)) + 2
    tw, th = x1 - x0 + 1, y1 - y0 + 1
    return x0, y0, tw, th, not (tw * th > cap or tw * th > 2 * ps * ps)
