"""Homography reprojection of LAFs and ground-truth correspondences with the reference's names
(ReprojectionStuff.py:23-40,126-137), plus the SNN matcher of train_AffNet_test_on_graffity.py:292-300 as one call, and the geometric
verification of its tentative matches from the affine frames themselves (csrc/spatial.hip: verify_matches, enqueue_verify, match_and_verify)."""
import ctypes as C

import numpy as np
import torch

from . import engine, _lib
from ._lib import lib, check, ptr


def _h9(H):
    h = np.ascontiguousarray(torch.as_tensor(H).detach().cpu().numpy(), dtype=np.float32).reshape(9)
    return (C.c_float * 9)(*h.tolist())


def reprojectLAFs(LAFs1, H1to2, return_LHFs=False):
    """Pixel LAFs (n,2,3) cuda -> reprojected LAFs (n,2,3) (or (n,3,3) homogeneous frames)."""
    engine.require_cuda(LAFs1, "LAFs1")
    lafs = LAFs1.contiguous().float()
    out = torch.empty_like(lafs)
    n = lafs.size(0)
    if n:
        ctx = engine.utility_ctx(lafs.device)
        check(lib.affnet_reproject_lafs(ctx, ptr(lafs), n, _h9(H1to2), ptr(out), engine.stream_of(lafs.device)), ctx, "affnet_reproject_lafs")
    if return_LHFs:
        last = torch.tensor([0.0, 0.0, 1.0], device=lafs.device).view(1, 1, 3).repeat(n, 1, 1)
        return torch.cat([out, last], dim=1)
    return out


def get_GT_correspondence_indexes(LAFs1, LAFs2, H1to2, dist_threshold=4):
    """ReprojectionStuff.py:126-137: (min_dist[mask], plain_indxs_in1[mask], idxs_in_2[mask])."""
    engine.require_cuda(LAFs1, "LAFs1")
    Hinv = torch.inverse(torch.as_tensor(H1to2).detach().cpu().float())        # 3x3 on the host, as the reference (LAPACK)
    l2_in_1 = reprojectLAFs(LAFs2, Hinv)
    l1 = LAFs1.contiguous().float()
    nq, nr = l1.size(0), l2_in_1.size(0)       # rows = image-1 LAFs, minimum over the reprojected image-2 LAFs (:131-132)
    dev = l1.device
    md = torch.empty(nq, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq and nr:
        ctx = engine.utility_ctx(dev)
        check(lib.affnet_centre_nn(ctx, ptr(l1), nq, ptr(l2_in_1), nr, ptr(md), ptr(idx), engine.stream_of(dev)), ctx, "affnet_centre_nn")
    mask = md <= dist_threshold
    plain = torch.arange(0, nq, device=dev)
    return md[mask], plain[mask], idx[mask].long()


def match_snn(descriptors1, descriptors2, SNN_threshold=0.8):
    """train_AffNet_test_on_graffity.py:292-300 in one fused call (no n1 x n2 matrix in HBM).
    Returns (tent_matches_in_1, tent_matches_in_2, min_dist, min_2nd_dist) - the first two int64 like the reference."""
    engine.require_cuda(descriptors1, "descriptors1")
    engine.require_cuda(descriptors2, "descriptors2")
    a, b = descriptors1.contiguous().float(), descriptors2.contiguous().float()
    n1, n2, dev = a.size(0), b.size(0), a.device
    if n2 == 0:
        raise ValueError("match_snn: descriptors2 is empty (the reference's torch.min over an empty dimension raises too)")
    if n1 == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return e, e.clone(), torch.empty(0, device=dev), torch.empty(0, device=dev)
    md = torch.empty(n1, dtype=torch.float32, device=dev)
    md2 = torch.empty(n1, dtype=torch.float32, device=dev)
    idx = torch.empty(n1, dtype=torch.int32, device=dev)
    tent = torch.empty(n1, 2, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=dev)
    ctx = engine.utility_ctx(dev)
    rc = lib.affnet_match_snn(ctx, ptr(a), n1, ptr(b), n2, a.size(1), float(SNN_threshold), ptr(md), ptr(idx), ptr(md2), ptr(tent), ptr(cnt),
                              ptr(scratch), engine.stream_of(dev))
    check(rc, ctx, "affnet_match_snn")
    k = int(cnt.item())
    return tent[:k, 0].long(), tent[:k, 1].long(), md, md2


VERIFY_MODELS = {"affine": _lib.VERIFY_AFFINE, "homography": _lib.VERIFY_HOMOGRAPHY}


def _verify_model(model):
    if model in VERIFY_MODELS:
        return VERIFY_MODELS[model]
    if model in (_lib.VERIFY_AFFINE, _lib.VERIFY_HOMOGRAPHY):
        return int(model)
    raise ValueError("model must be 'affine' or 'homography'")


def enqueue_verify(LAFs1, LAFs2, tent, count=None, inl_th=3.0, model="homography", lo_iters=3):
    """Spatial verification (affnet_verify_matches) of the tentative matches `tent` (cap,2) int32, of which the first count[0] rows are
    valid (count: (1,) int32 device tensor as affnet_match_snn writes it, or None = all rows), enqueued on the current stream with no
    synchronisation.  Returns capacity-sized device tensors: (H (3,3) float64, inliers (cap,) uint8, counts (cap,) int32, summary (4,)
    int32 = [best, counts[best], final inlier count, flags]); rows at or beyond the count are zero."""
    engine.require_cuda(LAFs1, "LAFs1")
    engine.require_cuda(LAFs2, "LAFs2")
    engine.require_cuda(tent, "tent")
    if tent.dtype != torch.int32 or tent.dim() != 2 or tent.size(1) != 2 or not tent.is_contiguous():
        raise ValueError("enqueue_verify: tent must be a contiguous (cap,2) int32 tensor")
    if count is not None and (count.dtype != torch.int32 or count.numel() != 1 or not count.is_cuda):
        raise ValueError("enqueue_verify: count must be a (1,) int32 device tensor or None")
    l1, l2 = LAFs1.contiguous().float(), LAFs2.contiguous().float()
    dev, cap = l1.device, tent.size(0)
    H = torch.zeros(3, 3, dtype=torch.float64, device=dev)
    inl = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
    counts = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
    summary = torch.zeros(4, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.affnet_verify_scratch_bytes(cap), dtype=torch.uint8, device=dev)
    one = torch.zeros(8, dtype=torch.float32, device=dev)           # stands in for an empty frame / match list: never read, but the boundary refuses NULL
    ctx = engine.utility_ctx(dev)
    rc = lib.affnet_verify_matches(ctx, ptr(l1 if l1.numel() else one), l1.size(0), ptr(l2 if l2.numel() else one), l2.size(0),
                                   ptr(tent if cap else one), ptr(count), cap, float(inl_th), _verify_model(model), int(lo_iters),
                                   ptr(counts), ptr(H), ptr(inl), ptr(summary), ptr(scratch), engine.stream_of(dev))
    check(rc, ctx, "affnet_verify_matches")
    return H, inl[:cap], counts[:cap], summary


def _verify_info(counts, summary_host):
    return {"counts": counts, "best": int(summary_host[0]), "best_count": int(summary_host[1]), "num_inliers": int(summary_host[2]),
            "flags": int(summary_host[3])}


def verify_matches(LAFs1, LAFs2, tent_in_1, tent_in_2, inl_th=3.0, model="homography", lo_iters=3):
    """Geometric verification of tentative matches without ground truth.  Every tentative (tent_in_1[t], tent_in_2[t]) - the index tensors
    match_snn returns - is one affine hypothesis LAFs2[j] LAFs1[i]^-1; all are scored against all matches (centre error <= inl_th px), the
    best one is refined by lo_iters least-squares refits of `model` ('homography' or 'affine') on its inliers.  Deterministic.
    Returns (H (3,3) float64 device tensor mapping image 1 to image 2, inliers (T,) bool, info) with info = {counts (T,) int32 inliers per
    hypothesis, best, best_count, num_inliers, flags: 1 no valid hypothesis, 2 too few inliers to refit, 4 degenerate system}."""
    engine.require_cuda(LAFs1, "LAFs1")
    tent = torch.stack([torch.as_tensor(tent_in_1, device=LAFs1.device).reshape(-1), torch.as_tensor(tent_in_2, device=LAFs1.device).reshape(-1)], 1)
    tent = tent.to(torch.int32).contiguous()
    H, inl, counts, summary = enqueue_verify(LAFs1, LAFs2, tent, None, inl_th, model, lo_iters)
    return H, inl.bool(), _verify_info(counts, summary.cpu().tolist())


def match_and_verify(descriptors1, descriptors2, LAFs1, LAFs2, SNN_threshold=0.8, inl_th=3.0, model="homography", lo_iters=3):
    """match_snn followed by verify_matches as one chain on the stream: the tentative list and its device-side count go from
    affnet_match_snn straight into affnet_verify_matches, and the host reads back once, at the end.
    Returns (tent_matches_in_1, tent_matches_in_2, H, inliers (T,) bool, info) - the pieces of match_snn and verify_matches."""
    engine.require_cuda(descriptors1, "descriptors1")
    engine.require_cuda(descriptors2, "descriptors2")
    a, b = descriptors1.contiguous().float(), descriptors2.contiguous().float()
    n1, n2, dev = a.size(0), b.size(0), a.device
    if n2 == 0:
        raise ValueError("match_and_verify: descriptors2 is empty")
    if LAFs1.size(0) != n1 or LAFs2.size(0) != n2:
        raise ValueError("match_and_verify: one LAF per descriptor row (%d / %d frames for %d / %d descriptors)" % (LAFs1.size(0), LAFs2.size(0), n1, n2))
    tent = torch.empty(n1, 2, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    if n1:
        md = torch.empty(n1, dtype=torch.float32, device=dev)
        md2 = torch.empty(n1, dtype=torch.float32, device=dev)
        idx = torch.empty(n1, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=dev)
        ctx = engine.utility_ctx(dev)
        rc = lib.affnet_match_snn(ctx, ptr(a), n1, ptr(b), n2, a.size(1), float(SNN_threshold), ptr(md), ptr(idx), ptr(md2), ptr(tent), ptr(cnt),
                                  ptr(scratch), engine.stream_of(dev))
        check(rc, ctx, "affnet_match_snn")
    H, inl, counts, summary = enqueue_verify(LAFs1, LAFs2, tent, cnt, inl_th, model, lo_iters)
    host = torch.cat([cnt, summary]).cpu().tolist()          # the one read-back
    k = host[0]
    return tent[:k, 0].long(), tent[:k, 1].long(), H, inl[:k].bool(), _verify_info(counts[:k], host[1:])
