"""Float64 restatements of the two hand-crafted slot fillers of csrc/handcrafted.hip (hc19_kernel<0> orientation, hc19_kernel<1>
Baumberg) and the deterministic 19 x 19 patch families that tests/test_handcrafted_host.py and tests/test_gpu_handcrafted.py run them
on.  numpy + oracle/affnet_oracle.py only: no affnet_amd, no GPU.

Orientation.  orientation_f64 follows orc.orientation_detector operation for operation in float64, with the two fp32 scalars that both
the reference and the kernel use (pi and 2 pi rounded to fp32) and the fp32 window 10 * circular_gauss_kernel(19) widened.  A pixel's bin
is floor(o_big): where o_big lies within TOL of an integer the bin hangs on the last ulps of atan2f, which the device and the host may
round differently, and the pixel's whole weight moves between two bins.  A patch is DECIDED iff
    top1 - top2 > 2 (0.34 u + 1e-5 top1),
top1 / top2 the two largest smoothed bins and u the sum of mag * gk / 361 over such pixels: no rounding of atan2f can then change the
argmax.  Every other patch must still get one of the restatement's two largest bins.

Baumberg.  baumberg_f64 is orc.affine_shape_estimator with every value in double (the fp32 window widened) and also returns the two
eigenvalues of the weighted second-moment matrix [[a, b], [b, c]]; values are compared only where the smaller eigenvalue is at least
COND times the larger one."""
import os

import numpy as np

import affnet_oracle as orc

PS = 19
N_BINS = 36
TOL = 1e-4
COND = 1e-3
PI32 = float(np.float32(np.pi))
TWO_PI32 = float(np.float32(2.0 * np.pi))
W_SIDE, W_MID = float(np.float32(0.33)), float(np.float32(0.34))          # the conv1d taps are fp32 tensors

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handcrafted_slots.npz")


def orientation_window():
    """(19, 19) float32: the reference's fp32 product 10 * float32(CircularGaussKernel(19)) (HandCraftedModules.py:152)."""
    return (np.float32(10.0) * orc.circular_gauss_kernel(kernlen=PS).astype(np.float32)).astype(np.float32)


def baumberg_window():
    """(19, 19) float32: CircularGaussKernel(19, sigma = 19 / 2 / 3) (HandCraftedModules.py:90)."""
    return orc.circular_gauss_kernel(kernlen=PS, sigma=(PS / 2) / 3.0).astype(np.float32)


def _neighbours(x):
    """x (n, 19, 19) float64 -> left, right, up, down neighbours under replicate padding."""
    xl = np.concatenate([x[:, :, :1], x[:, :, :-1]], axis=2)
    xr = np.concatenate([x[:, :, 1:], x[:, :, -1:]], axis=2)
    yu = np.concatenate([x[:, :1, :], x[:, :-1, :]], axis=1)
    yd = np.concatenate([x[:, 1:, :], x[:, -1:, :]], axis=1)
    return xl, xr, yu, yd


def orientation_f64(patches):
    """(n, 1, 19, 19) -> dict: bin (n,) the argmax (first maximum), hist (n, 36) the smoothed histogram, decided (n,) bool,
    top2 (n, 2) the two largest smoothed bins (stable: the lower bin first among equals), angle (n,) float32 as the kernel forms it."""
    x = np.asarray(patches, dtype=np.float64).reshape(-1, PS, PS)
    n = x.shape[0]
    gk = orientation_window().astype(np.float64)
    xl, xr, yu, yd = _neighbours(x)
    gx = 0.5 * xl - 0.5 * xr                                                   # taps [0.5, 0, -0.5]
    gy = 0.5 * yu - 0.5 * yd
    mag = np.sqrt(gx * gx + gy * gy + 1e-10) * gk
    ori = np.arctan2(gy, gx)
    o_big = float(N_BINS) * (ori + PI32) / TWO_PI32
    b0 = np.floor(o_big)
    w1 = o_big - b0
    b0 = np.mod(b0, float(N_BINS)).astype(np.int64)                            # numpy's mod is the floored one, like torch's %
    w0 = (1.0 - w1) * mag
    hist = np.zeros((n, N_BINS + 2))
    for i in range(N_BINS):
        hist[:, i + 1] = np.where(b0 == i, w0, 0.0).reshape(n, -1).sum(axis=1) / float(PS * PS)
    sm = W_SIDE * hist[:, :-2] + W_MID * hist[:, 1:-1] + W_SIDE * hist[:, 2:]  # conv1d, zero padding
    order = np.argsort(-sm, axis=1, kind="stable")
    top1, top2 = sm[np.arange(n), order[:, 0]], sm[np.arange(n), order[:, 1]]
    near = np.abs(o_big - np.round(o_big)) < TOL
    u = np.where(near, mag, 0.0).reshape(n, -1).sum(axis=1) / float(PS * PS)
    decided = (top1 - top2) > 2.0 * (W_MID * u + 1e-5 * top1)
    ang = -(((np.float32(TWO_PI32) * order[:, 0].astype(np.float32)) / np.float32(36.0)) - np.float32(PI32))
    return {"bin": order[:, 0].copy(), "hist": sm, "decided": decided, "top2": order[:, :2].copy(), "angle": ang.astype(np.float32),
            "n_near": near.reshape(n, -1).sum(axis=1)}


def bin_of_angle(angle):
    """The histogram bin an angle -(2 pi idx / 36 - pi) came from."""
    a = np.asarray(angle, dtype=np.float64)
    return np.round((PI32 - a) * N_BINS / TWO_PI32).astype(np.int64)


def baumberg_f64(patches):
    """(n, 1, 19, 19) -> (A (n, 2, 2) float64, eig (n, 2) float64 ascending): orc.affine_shape_estimator in double."""
    x = np.asarray(patches, dtype=np.float64).reshape(-1, PS, PS)
    n = x.shape[0]
    g = baumberg_window().astype(np.float64)
    xl, xr, yu, yd = _neighbours(x)
    gx, gy = xr - xl, yd - yu                                                  # taps [-1, 0, 1]
    a = (gx * gx * g).reshape(n, -1).mean(axis=1)
    b = (gx * gy * g).reshape(n, -1).mean(axis=1)
    c = (gy * gy * g).reshape(n, -1).mean(axis=1)
    half_tr, rad = 0.5 * (a + c), np.sqrt(0.25 * (a - c) ** 2 + b * b)
    eig = np.stack([half_tr - rad, half_tr + rad], axis=1)
    with np.errstate(all="ignore"):
        mask = (b != 0).astype(np.float64)
        r1 = mask * (c - a) / (2.0 * b + 1e-12)
        t1 = np.sign(r1) / (np.abs(r1) + np.sqrt(1.0 + r1 * r1))
        r = 1.0 / np.sqrt(1.0 + t1 * t1)
        t = t1 * r
        r = r * mask + 1.0 * (1.0 - mask)
        t = t * mask
        xx = 1.0 / np.sqrt(r * r * a - 2.0 * r * t * b + t * t * c)
        zz = 1.0 / np.sqrt(t * t * a + 2.0 * r * t * b + r * r * c)
        d = np.sqrt(xx * zz)
        xx, zz = xx / d, zz / d
        na = r * r * xx + t * t * zz
        nb = -r * t * xx + t * r * zz
        nc = t * t * xx + r * r * zz
        det = np.sqrt(np.abs(na * nc - nb * nb + 1e-10))                        # rectifyAffineTransformationUpIsUp of [[na, nb], [nb, nc]]
        b2a2 = np.sqrt(nb * nb + na * na)
        A = np.stack([np.stack([b2a2 / det, 0.0 * det], axis=1), np.stack([(nc * nb + nb * na) / (b2a2 * det), det / b2a2], axis=1)], axis=1)
    return A, eig


def well_conditioned(eig):
    return eig[:, 0] >= COND * eig[:, 1]


# ---- the input families ----------------------------------------------------------------------------------------------------------------
def families():
    """(patches (n, 1, 19, 19) float32, names list of n, family (n,) array of 'a' .. 'e')."""
    yy, xx = np.mgrid[0:PS, 0:PS].astype(np.float64)
    out, names, fam = [], [], []

    def add(p, name, f):
        out.append(np.asarray(p, dtype=np.float64).astype(np.float32)); names.append(name); fam.append(f)

    for k in range(N_BINS):                                                    # (a) ramps: the gradient direction sits mid-bin k
        t = (k + 0.5) * 2.0 * np.pi / N_BINS - np.pi
        add(128.0 - 40.0 * (np.cos(t) * (xx - 9.0) + np.sin(t) * (yy - 9.0)) / 9.0, "ramp%02d" % k, "a")
    rng = np.random.RandomState(1905)
    for k in range(100):                                                       # (b) uniform noise
        add(rng.uniform(0.0, 255.0, (PS, PS)), "noise%03d" % k, "b")
    rng = np.random.RandomState(1906)
    for k in range(100):                                                       # (c) anisotropic Gaussian blobs
        cx, cy = rng.uniform(4.0, 14.0, 2)
        s1, s2 = rng.uniform(1.5, 6.0, 2)
        th = rng.uniform(0.0, np.pi)
        u = np.cos(th) * (xx - cx) + np.sin(th) * (yy - cy)
        v = -np.sin(th) * (xx - cx) + np.cos(th) * (yy - cy)
        add(255.0 * np.exp(-0.5 * ((u / s1) ** 2 + (v / s2) ** 2)), "blob%03d" % k, "c")
    add(np.full((PS, PS), 77.0), "const77", "d")
    add(np.zeros((PS, PS)), "zero", "d")
    g = np.load(GOLDEN)["patches"].reshape(-1, PS, PS)
    for k in range(g.shape[0]):
        add(g[k], "golden%02d" % k, "e")
    return np.stack(out).reshape(-1, 1, PS, PS), names, np.array(fam)


def oracle_orientation_bins(patches):
    """Bins of the fp32 oracle (torch on the CPU)."""
    import torch
    return bin_of_angle(orc.orientation_detector(torch.from_numpy(np.ascontiguousarray(patches))).numpy())


def baumberg_reference_error(patches, fam):
    """{family: (e_ref, patches compared)}: max |orc.affine_shape_estimator (fp32) - float64 restatement| over the well-conditioned
    patches of families b, c, e.  The GPU test's bar is 8 x e_ref per family (the margin rule of tests/test_frames_host.py)."""
    import torch
    with np.errstate(all="ignore"):
        got = orc.affine_shape_estimator(torch.from_numpy(np.ascontiguousarray(patches))).numpy().astype(np.float64)
    want, eig = baumberg_f64(patches)
    ok = well_conditioned(eig)
    out = {}
    for f in "bce":
        sel = (fam == f) & ok
        out[f] = (float(np.abs(got[sel] - want[sel]).max()), int(sel.sum()))
    return out, got, want, eig
