"""float64 numpy restatement of SIFTNet(patch_size=32, num_ang_bins=8, num_spatial_bins=4).forward (pytorch_sift.py:69-94): the referee of
the SIFT tests.  Our own code: the steps are the ones a reader of the reference's forward() would list, evaluated in double.

  1. gradients by centred differences with replicate padding;
  2. mag = sqrt(gx^2 + gy^2 + 1e-10), ori = atan2(gy, gx + 1e-8);
  3. mag *= gk, the 32 x 32 circular Gaussian window (the float32 table, widened);
  4. soft binning: o = (ori + 2 pi) / (2 pi) * 8, b0 = floor(o), w1 = o - b0, bins b0 % 8 and (b0 + 1) % 8 get (1 - w1) mag and w1 mag;
  5. per bin an 11 x 11 stride-6 valid cross-correlation with the pooling table pk (float32 table, widened): 4 x 4 cells;
  6. flatten [bin][cy][cx];  7. L2 norm, clamp to [0, clipval], L2 norm (eps 1e-10 under the root, |sum|).

Against the reference's fp32 result on the 2 x 500 graf patches this differs by at most 1.93e-7 (tests/golden/make_golden_sift.py
stores the figure as ref_err_fp64): binning is continuous in o, so an fp32 / fp64 disagreement about floor(o) moves nothing."""
import numpy as np

PS, BINS, CELLS, KS, STRIDE = 32, 8, 4, 11, 6


def _l2norm(d):
    return d / np.sqrt(np.abs((d * d).sum(axis=1, keepdims=True)) + 1e-10)


def sift_fp64(patches, gk, pk, clipval=0.2):
    """patches (n,32,32) or (n,1,32,32), gk (32,32), pk (11,11) -> (n,128) float64."""
    p = np.asarray(patches, dtype=np.float64).reshape(-1, PS, PS)
    gk = np.asarray(gk, dtype=np.float64).reshape(PS, PS)
    pk = np.asarray(pk, dtype=np.float64).reshape(KS, KS)
    e = np.pad(p, ((0, 0), (1, 1), (1, 1)), mode="edge")
    gx = e[:, 1:-1, 2:] - e[:, 1:-1, :-2]
    gy = e[:, 2:, 1:-1] - e[:, :-2, 1:-1]
    mag = np.sqrt(gx * gx + gy * gy + 1e-10) * gk
    ori = np.arctan2(gy, gx + 1e-8)
    o = (ori + 2.0 * np.pi) / (2.0 * np.pi) * BINS
    b0 = np.floor(o)
    w1 = o - b0
    b0 = np.mod(b0, BINS)
    b1 = np.mod(b0 + 1, BINS)
    w0m, w1m = (1.0 - w1) * mag, w1 * mag
    out = np.zeros((p.shape[0], BINS, CELLS, CELLS))
    for i in range(BINS):
        m = (b0 == i) * w0m + (b1 == i) * w1m
        for cy in range(CELLS):
            for cx in range(CELLS):
                out[:, i, cy, cx] = (m[:, STRIDE * cy:STRIDE * cy + KS, STRIDE * cx:STRIDE * cx + KS] * pk).sum(axis=(1, 2))
    d = _l2norm(out.reshape(p.shape[0], -1))
    d = np.clip(d, 0.0, float(clipval))
    return _l2norm(d)
