"""Shared by tests/test_gpu_frames.py and tests/test_frames_host.py (not a test module): the float64 restatement of ells2LAFsT that the
ellipse bars are derived from, and the oracle side of "frames the detector never produced" (computed once per session)."""
import os

import numpy as np
import torch

import affnet_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, W = 240, 320
MR, BORDER = 3.0, 16          # the extractor's constructor defaults


# ---- ellipses -----------------------------------------------------------------------------------------------------------------
def ells2lafs_f64(ells):
    """LAF.py:76-89 (ells2LAFsT) with invSqrtTorch (:52-74) and rectifyAffineTransformationUpIsUp (:285-291), the same formulas in
    float64 numpy: what the fp32 reference output is an approximation OF."""
    e = np.asarray(ells, dtype=np.float64)
    a, b, c = e[:, 2], e[:, 3], e[:, 4]
    sc = np.sqrt(np.sqrt(a * c - b * b + 1e-12))
    mask = (b != 0).astype(np.float64)
    r1 = mask * (c - a) / (2.0 * b + 1e-12)
    t1 = np.sign(r1) / (np.abs(r1) + np.sqrt(1.0 + r1 * r1))
    r = 1.0 / np.sqrt(1.0 + t1 * t1)
    t = t1 * r
    r = r * mask + 1.0 * (1.0 - mask)
    t = t * mask
    x = 1.0 / np.sqrt(r * r * a - 2.0 * r * t * b + t * t * c)
    z = 1.0 / np.sqrt(t * t * a + 2.0 * r * t * b + r * r * c)
    d = np.sqrt(x * z)
    x, z = x / d, z / d
    ia, ib, ic = r * r * x + t * t * z, -r * t * x + t * r * z, t * t * x + r * r * z
    A = np.stack([np.stack([ia / sc, ib / sc], 1), np.stack([ib / sc, ic / sc], 1)], 1)
    sc2 = np.sqrt(np.abs(A[:, 0, 0] * A[:, 1, 1] - A[:, 1, 0] * A[:, 0, 1]))
    Bm = A / sc2[:, None, None]
    det = np.sqrt(np.abs(Bm[:, 0, 0] * Bm[:, 1, 1] - Bm[:, 1, 0] * Bm[:, 0, 1] + 1e-10))
    b2a2 = np.sqrt(Bm[:, 0, 1] ** 2 + Bm[:, 0, 0] ** 2)
    out = np.zeros((len(e), 2, 3))
    out[:, 0, 0] = b2a2 / det * sc2
    out[:, 1, 0] = (Bm[:, 1, 1] * Bm[:, 0, 1] + Bm[:, 1, 0] * Bm[:, 0, 0]) / (b2a2 * det) * sc2
    out[:, 1, 1] = det / b2a2 * sc2
    out[:, 0, 2], out[:, 1, 2] = e[:, 0], e[:, 1]
    return out


def shape_err(lafs, want):
    """max |delta| of the 2x2 part over the frame scale sqrt|det| of `want`, per row."""
    lafs, want = np.asarray(lafs, dtype=np.float64), np.asarray(want, dtype=np.float64)
    S = np.sqrt(np.abs(want[:, 0, 0] * want[:, 1, 1] - want[:, 0, 1] * want[:, 1, 0]))
    return np.abs(lafs[:, :, :2] - want[:, :, :2]).reshape(len(want), -1).max(axis=1) / S


def ell_rel_err(ell, want):
    """max |delta| of (a, b, c) over the row's largest coefficient, per row."""
    ell, want = np.asarray(ell, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(ell[:, 2:] - want[:, 2:]).max(axis=1) / np.abs(want[:, 2:]).max(axis=1)


def golden_ells():
    """(ells, lafs, bar_shape, bar_roundtrip, measured): the fixture and the two bars, each 8 x the reference's OWN error on it - its fp32
    output against the float64 restatement, and its own fp32 round trip LAFs2ellT(ells2LAFsT(e)) against e (tests/test_gpu_sift.py's
    precedent for "another fp32 rounding of the same formula")."""
    g = np.load(os.path.join(GOLDEN, "ells2lafs.npz"))
    ells, lafs = g["ells"], g["lafs"]
    own = float(shape_err(lafs, ells2lafs_f64(ells)).max())
    back = orc.lafs_to_ellipses_t(torch.from_numpy(lafs)).numpy()
    own_rt = float(ell_rel_err(back, ells).max())
    return ells, lafs, 8.0 * own, 8.0 * own_rt, {"reference_own_error": own, "reference_own_round_trip": own_rt}


# ---- frames the detector never produced ------------------------------------------------------------------------------------------
_CACHE = {}


def foreign_frames(weights):
    """The oracle's 450 candidates of the 240x320 synthetic image (seed 1), denormalised, permuted, sheared, rotated and rescaled:
    pixel frames (450,2,3), distinct unsorted responses (450,), and the OracleExtractor that holds the pyramid."""
    if "frames" not in _CACHE:
        x = orc.synthetic_image(H, W, 1)
        ex = orc.OracleExtractor(mrSize=MR, num_features=300, border=BORDER, num_Baum_iters=1, affnet_sd=weights["AffNet"], orinet_sd=weights["OriNet"])
        ex(x, do_ori=False)
        fr = orc.denormalize_lafs(ex.detected["lafs"], W, H)
        n = fr.size(0)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(7))
        fr = fr[perm].clone()
        i = torch.arange(n, dtype=torch.float32)
        shear = torch.tensor([[1.0, 0.0], [0.25, 0.9]]).expand(n, 2, 2)
        scale = torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.arange(n) % 4]
        A = torch.bmm(torch.bmm(fr[:, :, :2], shear), orc.rotation_matrix(0.37 * i)) * scale.view(-1, 1, 1)
        fr = torch.cat([A, fr[:, :, 2:]], dim=2).contiguous()
        resp = (perm + 1).float() * 0.125
        _CACHE["frames"] = (x, ex, fr, resp)
    return _CACHE["frames"]


def oracle_on_frames(weights, n_out):
    """Unchanged oracle stages on the foreign frames: level rule at PS 32, AffNet shape + filter + top-n_out, OriNet, HardNet."""
    key = ("oracle", n_out)
    if key not in _CACHE:
        x, ex, fr, resp = foreign_frames(weights)
        with torch.no_grad():
            octs, levs = ex.level_for_lafs(fr, 32)
            det = {"resp": resp.clone(), "lafs": orc.normalize_lafs(fr, W, H), "oct": octs, "lev": levs, "pix": torch.arange(fr.size(0))}
            r, lafs, o, l, rows = ex._affine_shape(det, n_out)
            stage = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in ex.shape_stage.items()}
            lafs = ex._orientation(lafs, o, l)
            ori = ex.ori_vec.clone()
            px = orc.denormalize_lafs(lafs, W, H)
            desc = orc.hardnet_forward(weights["HardNet"], ex.extract_patches_from_pyr(px, PS=32))
        _CACHE[key] = {"resp": r.numpy(), "LAFs": px.numpy(), "rows": rows.numpy(), "desc": desc.numpy(), "ori_vec": ori.numpy(), "stage": stage,
                       "oct": octs.numpy(), "lev": levs.numpy()}
    return _CACHE[key]


def margins(stage):
    """How far the oracle's shape decisions on the foreign frames are from flipping.  Eigenvalue ratio: log distance from 6 and 1/6.
    Boundary test: for a frame inside the image the smallest distance of a corner coordinate from the border, for a frame outside the
    largest overshoot of one (what decides that row), in normalised units."""
    lr = np.log(stage["ratio"].numpy().astype(np.float64))
    ratio_margin = float(np.minimum(np.abs(lr - np.log(6.0)), np.abs(lr + np.log(6.0))).min())
    c = orc.frame_corners(stage["frames"]).numpy().astype(np.float64).reshape(len(lr), -1)
    inside = np.minimum(c, 1.0 - c)                    # > 0: that coordinate is inside
    row = np.where(inside.min(axis=1) >= 0, inside.min(axis=1), -inside.min(axis=1))
    return ratio_margin, float(row.min())
