"""Python mirror of the margin rule of the fused AffNet shape pass (affnet_amd/csrc/shape_filter.h: aff_shape_margin_flag, shape form 1 of
affnet_set_shape_form) and of what surrounds it: A from the pooled head outputs as affnet_finish_kernel forms it (cnn_heads.hip) and the shape filter's
decision (aff_shape_filter_row), all in fp32, operation by operation; fmaf(a, b, c) is the float64 product and sum rounded to fp32.  Shared by
tests/test_shape_margin.py (CPU: the oracle's candidates through the direct and the Winograd fp32 mirrors of tools/winograd_numerics.py) and
tests/test_gpu_shape_form.py (the rule applied to the library's own A and frames)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402
import winograd_numerics as wn  # noqa: E402

DELTA = 4e-6                 # assumed bound on |Winograd - direct| per pooled head output (shape_filter.h)
MARGIN_D1 = np.float32(1e-5)
MARGIN_CORNER = np.float32(1e-5)
MARGIN_RATIO_REL = np.float32(1e-3)
FLAGGED_SHARE_CAP = 0.05     # cap on the flagged share per image (the reference alone: 1.3 - 2.9 % on the 320x240 synthetic images)
H, W, N_FEATURES = 240, 320, 300
MR_SIZE, BORDER = 5.192, 5   # the benchmark's extractor settings
f32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def candidates(sd, seed):
    """The oracle's candidates of the synthetic 320x240 image `seed` (num_features 300 -> 450 candidates): (patches (n,1,32,32), normalised frames (n,2,3))"""
    ex = orc.OracleExtractor(num_features=N_FEATURES, num_Baum_iters=1, affnet_sd=sd, mrSize=MR_SIZE, border=BORDER)
    ex(orc.synthetic_image(H, W, seed))
    d = ex.detected
    with torch.no_grad():
        patches = orc.extract_from_pyramid(ex.scale_pyr, d["oct"], d["lev"], d["lafs"], 32)
    return patches, d["lafs"].clone()


def heads(sd, patches):
    """Pooled head outputs (n, 3) of the direct fp32 trunk and of the one with conv1 / conv3 as Winograd"""
    with torch.no_grad():
        out = []
        for layers in ((), (1, 3)):
            y = wn.trunk16_layers(sd, patches, layers)[5]
            out.append(wn.head16(sd, y, "affnet").numpy().astype(f32))
    return out


def a_from_head(x):
    """affnet_finish_kernel: [[1 + x0, 0 * x0], [x1, 1 + x2]] -> rectifyAffineTransformationUpIsUp; (n, 4) = (o0, o1, o2, o3)"""
    x = np.asarray(x, dtype=f32)
    one, zero = f32(1.0), f32(0.0)
    a00, a01, a10, a11 = one + x[:, 0], zero * x[:, 0], x[:, 1], one + x[:, 2]
    det = np.sqrt(np.abs(a00 * a11 - a10 * a01 + f32(1e-10)))
    b2a2 = np.sqrt(a01 * a01 + a00 * a00)
    return np.stack([b2a2 / det, zero * det, (a11 * a01 + a10 * a00) / (b2a2 * det), det / b2a2], axis=1).astype(f32)


def _terms(A, lafs):
    """What both the filter and the rule look at: (d1, ratio, corner coordinates (n, 8))"""
    A = np.asarray(A, dtype=f32)
    L = np.asarray(lafs, dtype=f32).reshape(-1, 6)
    a00, a01, a10, a11 = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    n00, n01 = _fma(a01, L[:, 3], a00 * L[:, 0]), _fma(a01, L[:, 4], a00 * L[:, 1])
    n10, n11 = _fma(a11, L[:, 3], a10 * L[:, 0]), _fma(a11, L[:, 4], a10 * L[:, 1])
    cx, cy = L[:, 2], L[:, 5]
    tr = a00 + a11
    p1, p2 = a00 * a11, a10 * a01
    d1 = tr * tr - f32(4.0) * (p1 - p2)
    mk = (d1 > 0).astype(f32)
    dl = np.sqrt(np.abs(d1))
    l1 = mk * (tr + dl) / f32(2.0) + f32(1000.0) * (f32(1.0) - mk)
    l2 = mk * (tr - dl) / f32(2.0) + f32(0.0001) * (f32(1.0) - mk)
    ratio = np.abs(l1 / (l2 + f32(1e-8)))
    one = np.ones_like(cx)
    corners = []
    for px, py in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
        corners.append(_fma(cx, one, _fma(n01, f32(py) * one, n00 * f32(px))))
        corners.append(_fma(cy, one, _fma(n11, f32(py) * one, n10 * f32(px))))
    return d1, ratio, np.stack(corners, axis=1)


def filter_decision(A, lafs):
    """aff_shape_filter_row: the row's `good` flag"""
    with np.errstate(all="ignore"):
        _, ratio, c = _terms(A, lafs)
        return (ratio < f32(6.0)) & (ratio > f32(1.0 / 6.0)) & ~((c > f32(1.0)) | (c < f32(0.0))).any(axis=1)


def margin_flag(A, lafs):
    """aff_shape_margin_flag: True = not certain, the direct trunk recomputes the row"""
    with np.errstate(all="ignore"):
        A = np.asarray(A, dtype=f32)
        _, ratio, c = _terms(A, lafs)
        iso = (A[:, 0] - A[:, 3]) * (A[:, 0] - A[:, 3])
        certain = (iso >= MARGIN_D1) & (np.abs(ratio - f32(6.0)) >= f32(6.0) * MARGIN_RATIO_REL) & \
                  (np.abs(ratio - f32(1.0 / 6.0)) >= MARGIN_RATIO_REL / f32(6.0))
        certain &= ((np.abs(c) >= MARGIN_CORNER) & (np.abs(c - f32(1.0)) >= MARGIN_CORNER)).all(axis=1)
        return ~certain
