"""Homography reprojection of LAFs and ground-truth correspondences with the reference's names
(ReprojectionStuff.py:23-40,126-137), plus the SNN matcher of train_AffNet_test_on_graffity.py:292-300 as one call, and the geometric
verification of its tentative matches from the affine frames themselves (csrc/spatial.hip: verify_matches, enqueue_verify, match_and_verify), and both for many image pairs per device call (pair_table,
enqueue_match_and_verify_many, match_and_verify_many, spatial_rerank).  The epipolar model of a scene with depth is csrc/epipolar.hip
(verify_epipolar, enqueue_verify_epipolar, model="fundamental" of verify_matches / match_and_verify, sampson_distance); its plane-aware form for scenes whose matches lie mostly on one plane is csrc/epipolar_planar.hip (verify_epipolar_planar,
enqueue_verify_epipolar_planar, model="fundamental_planar" of the single-pair functions).  Guided matching under a
verified model of either family is csrc/guided.hip (match_guided, enqueue_match_guided, guided_mask, match_verify_guided).  Both have their
many-pairs form too (affnet_epipolar_verify_many, affnet_match_guided_many): model="fundamental" of the *_many functions,
enqueue_match_verify_guided_many, match_verify_guided_many, guided=True of spatial_rerank.  The ratio-test matcher with a per-row second
neighbour, FGINN and a mutual check is csrc/ratio_match.hip (match_ratio, match_fginn, enqueue_match_ratio, matcher="snn" / "fginn" of the
match-and-verify chains)."""
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


# ---- ratio-test matching (csrc/ratio_match.hip: affnet_match_ratio, affnet_match_ratio_many) -----------------------------------------------------

MATCHERS = ("reference", "snn", "fginn")


def _matcher_radius(what, matcher, fginn_radius, mutual=False, guided=False):
    """The radius affnet_match_ratio takes for `matcher` ('snn': -1, 'fginn': fginn_radius), None for 'reference' (affnet_match_snn)."""
    if matcher not in MATCHERS:
        raise ValueError("%s: matcher must be 'reference', 'snn' or 'fginn'" % what)
    if matcher == "reference":
        if mutual:
            raise ValueError("%s: the reference matcher has no mutual check (matcher='snn' or 'fginn')" % what)
        return None
    if guided:
        raise ValueError("%s: the guided chains keep the reference matcher as their first stage" % what)
    if matcher == "snn":
        return -1.0
    r = float(np.float32(fginn_radius))
    if not (np.isfinite(r) and r >= 0):
        raise ValueError("%s: fginn_radius must be a finite number >= 0" % what)
    return r


def enqueue_match_ratio(desc1, desc2, LAFs2=None, radius=None, SNN_threshold=0.8, max_dist=float("inf"), mutual=False, n_chunks=0):
    """Ratio-test matching (affnet_match_ratio) enqueued on the current stream with no synchronisation.  Every row of desc1 takes its nearest
    row of desc2 and, as the second distance of the ratio, the nearest OTHER row - radius None or < 0, Lowe's test - or the nearest row whose
    frame centre lies more than `radius` px from the nearest one's (radius >= 0, needs LAFs2: the first geometrically inconsistent neighbour).
    A pair is kept when its distance is <= max_dist, the ratio is <= SNN_threshold and, with `mutual`, the row is also the nearest row of its
    column.
    Returns capacity-sized device tensors (tent (n1,2) int32, count (1,) int32, dist (n1,2), idx (n1,2) int32: the two slots per row,
    (+inf, -1) where there is none); rows of tent at or beyond the count are zero."""
    engine.require_cuda(desc1, "desc1")
    engine.require_cuda(desc2, "desc2")
    a, b = desc1.contiguous().float(), desc2.contiguous().float()
    n1, n2, dev = a.size(0), b.size(0), a.device
    radius = -1.0 if radius is None else float(radius)
    l2 = None
    if radius >= 0:
        if LAFs2 is None:
            raise ValueError("enqueue_match_ratio: a radius >= 0 needs LAFs2")
        engine.require_cuda(LAFs2, "LAFs2")
        if LAFs2.numel() != 6 * n2:
            raise ValueError("enqueue_match_ratio: one LAF per row of desc2 (%d frames for %d descriptors)" % (LAFs2.numel() // 6, n2))
        l2 = LAFs2.contiguous().float()
    tent = torch.zeros(max(n1, 1), 2, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    dist = torch.full((max(n1, 1), 2), float("inf"), dtype=torch.float32, device=dev)
    idx = torch.full((max(n1, 1), 2), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.affnet_match_ratio_scratch_bytes(n1, n2, int(n_chunks)), dtype=torch.uint8, device=dev)
    one = torch.zeros(8, dtype=torch.float32, device=dev)           # stands in for an empty side: never read, but the boundary refuses NULL
    ctx = engine.utility_ctx(dev)
    rc = lib.affnet_match_ratio(ctx, ptr(a if n1 else one), n1, ptr(b if n2 else one), n2, a.size(1), ptr(one if l2 is not None and not n2 else l2), radius,
                                float(SNN_threshold), float(max_dist), _lib.RATIO_MUTUAL if mutual else 0, int(n_chunks), ptr(dist), ptr(idx), ptr(tent),
                                ptr(cnt), ptr(scratch), engine.stream_of(dev))
    check(rc, ctx, "affnet_match_ratio")
    return tent[:n1], cnt, dist[:n1], idx[:n1]


def match_ratio(desc1, desc2, LAFs2=None, radius=None, SNN_threshold=0.8, max_dist=float("inf"), mutual=False, n_chunks=0):
    """enqueue_match_ratio and one read-back.  Returns (tent_matches_in_1, tent_matches_in_2, dist (n1,2), idx (n1,2)) - the first two int64, as
    match_snn returns them.  radius=None means -1: the plain per-row ratio test."""
    tent, cnt, dist, idx = enqueue_match_ratio(desc1, desc2, LAFs2, radius, SNN_threshold, max_dist, mutual, n_chunks)
    k = int(cnt.item())
    return tent[:k, 0].long(), tent[:k, 1].long(), dist, idx


def match_fginn(desc1, desc2, LAFs2, radius=10.0, SNN_threshold=0.8, max_dist=float("inf"), mutual=False, n_chunks=0):
    """match_ratio with the radius of MODS: the ratio is taken against the nearest descriptor whose centre lies more than 10 px from the nearest
    neighbour's, so a second detection of the same structure does not refuse a good match."""
    return match_ratio(desc1, desc2, LAFs2, radius, SNN_threshold, max_dist, mutual, n_chunks)


VERIFY_MODELS = {"affine": _lib.VERIFY_AFFINE, "homography": _lib.VERIFY_HOMOGRAPHY}


def _verify_model(model):
    if model in VERIFY_MODELS:
        return VERIFY_MODELS[model]
    if model in (_lib.VERIFY_AFFINE, _lib.VERIFY_HOMOGRAPHY):
        return int(model)
    raise ValueError("model must be 'affine' or 'homography' ('fundamental': verify_matches, match_and_verify, verify_epipolar)")


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


def _tent_tensor(LAFs1, tent_in_1, tent_in_2):
    tent = torch.stack([torch.as_tensor(tent_in_1, device=LAFs1.device).reshape(-1), torch.as_tensor(tent_in_2, device=LAFs1.device).reshape(-1)], 1)
    return tent.to(torch.int32).contiguous()


def verify_matches(LAFs1, LAFs2, tent_in_1, tent_in_2, inl_th=3.0, model="homography", lo_iters=3, rounds=8, seed=0, plane_th=3.0):
    """Geometric verification of tentative matches without ground truth.  Every tentative (tent_in_1[t], tent_in_2[t]) - the index tensors
    match_snn returns - is one affine hypothesis LAFs2[j] LAFs1[i]^-1; all are scored against all matches (centre error <= inl_th px), the
    best one is refined by lo_iters least-squares refits of `model` ('homography' or 'affine') on its inliers.  Deterministic.
    Returns (H (3,3) float64 device tensor mapping image 1 to image 2, inliers (T,) bool, info) with info = {counts (T,) int32 inliers per
    hypothesis, best, best_count, num_inliers, flags: 1 no valid hypothesis, 2 too few inliers to refit, 4 degenerate system}.
    model='fundamental' is verify_epipolar (a scene with depth; `rounds` and `seed` are read by that model only); model='fundamental_planar' is
    verify_epipolar_planar (a scene with depth whose matches lie mostly on one plane; it alone reads `plane_th`)."""
    engine.require_cuda(LAFs1, "LAFs1")
    if model == "fundamental":
        return verify_epipolar(LAFs1, LAFs2, tent_in_1, tent_in_2, inl_th, rounds, seed, lo_iters)
    if model == "fundamental_planar":
        return verify_epipolar_planar(LAFs1, LAFs2, tent_in_1, tent_in_2, inl_th, plane_th, rounds, seed, lo_iters)
    H, inl, counts, summary = enqueue_verify(LAFs1, LAFs2, _tent_tensor(LAFs1, tent_in_1, tent_in_2), None, inl_th, model, lo_iters)
    return H, inl.bool(), _verify_info(counts, summary.cpu().tolist())


def enqueue_verify_epipolar(LAFs1, LAFs2, tent, count=None, inl_th=2.0, rounds=8, seed=0, lo_iters=3):
    """Epipolar verification (affnet_epipolar_verify) of the tentative matches `tent` (cap,2) int32, of which the first count[0] rows are valid
    (count: (1,) int32 device tensor as affnet_match_snn writes it, or None = all rows), enqueued on the current stream with no synchronisation.
    Returns capacity-sized device tensors: (F (3,3) float64 with x2^T F x1 = 0, inliers (cap,) uint8, counts (cap*rounds,) int32 inliers per
    hypothesis h = s * rounds + r, summary (4,) int32 = [best, counts[best], final inlier count, flags]); rows at or beyond the count are zero."""
    engine.require_cuda(LAFs1, "LAFs1")
    engine.require_cuda(LAFs2, "LAFs2")
    engine.require_cuda(tent, "tent")
    if tent.dtype != torch.int32 or tent.dim() != 2 or tent.size(1) != 2 or not tent.is_contiguous():
        raise ValueError("enqueue_verify_epipolar: tent must be a contiguous (cap,2) int32 tensor")
    if count is not None and (count.dtype != torch.int32 or count.numel() != 1 or not count.is_cuda):
        raise ValueError("enqueue_verify_epipolar: count must be a (1,) int32 device tensor or None")
    rounds, seed = int(rounds), int(seed)
    if not 1 <= rounds <= _lib.EPI_MAX_ROUNDS:
        raise ValueError("enqueue_verify_epipolar: rounds must be in 1..%d" % _lib.EPI_MAX_ROUNDS)
    if not 0 <= seed < 2 ** 32:
        raise ValueError("enqueue_verify_epipolar: seed must fit 32 unsigned bits")
    l1, l2 = LAFs1.contiguous().float(), LAFs2.contiguous().float()
    dev, cap = l1.device, tent.size(0)
    F = torch.zeros(3, 3, dtype=torch.float64, device=dev)
    inl = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
    counts = torch.zeros(max(cap * rounds, 1), dtype=torch.int32, device=dev)
    summary = torch.zeros(4, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.affnet_epipolar_scratch_bytes(cap, rounds), dtype=torch.uint8, device=dev)
    one = torch.zeros(8, dtype=torch.float32, device=dev)           # stands in for an empty frame / match list: never read, but the boundary refuses NULL
    ctx = engine.utility_ctx(dev)
    rc = lib.affnet_epipolar_verify(ctx, ptr(l1 if l1.numel() else one), l1.size(0), ptr(l2 if l2.numel() else one), l2.size(0),
                                    ptr(tent if cap else one), ptr(count), cap, float(inl_th), rounds, seed, int(lo_iters),
                                    ptr(counts), ptr(F), ptr(inl), ptr(summary), ptr(scratch), engine.stream_of(dev))
    check(rc, ctx, "affnet_epipolar_verify")
    return F, inl[:cap], counts[:cap * rounds], summary


def verify_epipolar(LAFs1, LAFs2, tent_in_1, tent_in_2, inl_th=2.0, rounds=8, seed=0, lo_iters=3):
    """Epipolar verification of tentative matches: for two views of a scene with depth, where one homography explains only the dominant plane.
    A frame is three point correspondences, so tentative s and two partners chosen by an integer hash of (s, r, seed) give one 8-point
    hypothesis; all T * rounds of them are scored against all matches (Sampson error of the centres <= inl_th px), the best one is refined by
    lo_iters rank-2 least-squares refits on its inliers.  Deterministic: the same bytes on every run.
    Returns (F (3,3) float64 device tensor, unit Frobenius norm, x2^T F x1 = 0; inliers (T,) bool; info) with the keys of verify_matches
    (counts has T * rounds entries, best = s * rounds + r; flag 1 comes with an all-zero F) plus rounds and seed.
    When most matches lie on one plane F is one of a family; it is then good as an inlier test only."""
    engine.require_cuda(LAFs1, "LAFs1")
    F, inl, counts, summary = enqueue_verify_epipolar(LAFs1, LAFs2, _tent_tensor(LAFs1, tent_in_1, tent_in_2), None, inl_th, rounds, seed, lo_iters)
    return F, inl.bool(), dict(_verify_info(counts, summary.cpu().tolist()), rounds=int(rounds), seed=int(seed))


def enqueue_verify_epipolar_planar(LAFs1, LAFs2, tent, count=None, inl_th=2.0, plane_th=3.0, rounds=8, seed=0, lo_iters=3):
    """Plane-aware epipolar verification (affnet_epipolar_verify_planar) of the tentative matches `tent`, with the arguments of
    enqueue_verify_epipolar plus plane_th, enqueued on the current stream with no synchronisation.  Returns capacity-sized device tensors:
    enqueue_verify_epipolar's four (F, inliers, counts, summary - summary[3] carries flag 16 when the plane-and-parallax model was kept),
    then H (3,3) float64 of the dominant plane, plane_inliers (cap,) uint8, plane_summary (4,) int32 and planar_info (4,) int32 =
    [matches off the plane, best plane-and-parallax hypothesis, its count, its final inlier count].
    counts is always the 8-point call's (cap*rounds entries, h = s * rounds + r over the tentatives).  With flag 16, summary[0] and summary[1]
    are the best PLANE-AND-PARALLAX hypothesis (h = a * rounds + r over the off-plane list) and its count: they do not index counts then."""
    engine.require_cuda(LAFs1, "LAFs1")
    engine.require_cuda(LAFs2, "LAFs2")
    engine.require_cuda(tent, "tent")
    if tent.dtype != torch.int32 or tent.dim() != 2 or tent.size(1) != 2 or not tent.is_contiguous():
        raise ValueError("enqueue_verify_epipolar_planar: tent must be a contiguous (cap,2) int32 tensor")
    if count is not None and (count.dtype != torch.int32 or count.numel() != 1 or not count.is_cuda):
        raise ValueError("enqueue_verify_epipolar_planar: count must be a (1,) int32 device tensor or None")
    rounds, seed = int(rounds), int(seed)
    if not 1 <= rounds <= _lib.EPI_MAX_ROUNDS:
        raise ValueError("enqueue_verify_epipolar_planar: rounds must be in 1..%d" % _lib.EPI_MAX_ROUNDS)
    if not 0 <= seed < 2 ** 32:
        raise ValueError("enqueue_verify_epipolar_planar: seed must fit 32 unsigned bits")
    l1, l2 = LAFs1.contiguous().float(), LAFs2.contiguous().float()
    dev, cap = l1.device, tent.size(0)
    F = torch.zeros(3, 3, dtype=torch.float64, device=dev)
    H = torch.zeros(3, 3, dtype=torch.float64, device=dev)
    inl = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
    pinl = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
    counts = torch.zeros(max(cap * rounds, 1), dtype=torch.int32, device=dev)
    ints = torch.zeros(3, 4, dtype=torch.int32, device=dev)          # summary, plane summary, planar info
    scratch = torch.empty(lib.affnet_epipolar_planar_scratch_bytes(cap, rounds), dtype=torch.uint8, device=dev)
    one = torch.zeros(8, dtype=torch.float32, device=dev)           # stands in for an empty frame / match list: never read, but the boundary refuses NULL
    ctx = engine.utility_ctx(dev)
    rc = lib.affnet_epipolar_verify_planar(ctx, ptr(l1 if l1.numel() else one), l1.size(0), ptr(l2 if l2.numel() else one), l2.size(0),
                                           ptr(tent if cap else one), ptr(count), cap, float(inl_th), float(plane_th), rounds, seed, int(lo_iters),
                                           ptr(counts), ptr(F), ptr(inl), ptr(ints[0]), ptr(H), ptr(pinl), ptr(ints[1]), ptr(ints[2]), ptr(scratch),
                                           engine.stream_of(dev))
    check(rc, ctx, "affnet_epipolar_verify_planar")
    return F, inl[:cap], counts[:cap * rounds], ints[0], H, pinl[:cap], ints[1], ints[2]


def _planar_info(info, H, plane_inliers, n_off):
    info.update(planar=bool(info["flags"] & _lib.EPI_FLAG_PLANAR), H=H, plane_inliers=plane_inliers.bool(), n_off_plane=int(n_off))
    return info


def verify_epipolar_planar(LAFs1, LAFs2, tent_in_1, tent_in_2, inl_th=2.0, plane_th=3.0, rounds=8, seed=0, lo_iters=3):
    """verify_epipolar for the scene that defeats it: a wall with a few things in front of it, where most matches lie on one plane and the
    8-point F is one of a family.  The dominant plane's homography H is found first (verify_matches, plane_th px); every match off that plane
    gives a line through the epipole, two lines give it, F = [e]x H; all (matches off the plane) * rounds such hypotheses are scored against
    all matches and the best is refitted on its inliers off the plane.  The result is this model when it has strictly more inliers than
    verify_epipolar's, else verify_epipolar's own bytes.  Deterministic.
    Returns (F, inliers, info) as verify_epipolar, with info additionally holding planar (bool: the plane-and-parallax model was kept;
    flags then carries 16), H (3,3) float64 device tensor, plane_inliers (T,) bool and n_off_plane.
    info["counts"] is always the 8-point model's per-hypothesis counts.  When planar is True, best and best_count describe the best
    plane-and-parallax hypothesis (a * rounds + r over the matches off the plane, in ascending order) instead, so counts[best] is not
    best_count then."""
    engine.require_cuda(LAFs1, "LAFs1")
    F, inl, counts, summary, H, pinl, _, pinfo = enqueue_verify_epipolar_planar(LAFs1, LAFs2, _tent_tensor(LAFs1, tent_in_1, tent_in_2), None, inl_th, plane_th,
                                                                                  rounds, seed, lo_iters)
    host = torch.cat([summary, pinfo]).cpu().tolist()
    return F, inl.bool(), _planar_info(dict(_verify_info(counts, host[:4]), rounds=int(rounds), seed=int(seed)), H, pinl, host[4])


def sampson_distance(F, LAFs1, LAFs2, tent_in_1, tent_in_2):
    """Square root of the Sampson error (pixels) of every tentative match's two centres under F (x2^T F x1 = 0): (T,) float64 on LAFs1's device."""
    F = torch.as_tensor(F, dtype=torch.float64, device=LAFs1.device).reshape(3, 3)
    i = torch.as_tensor(tent_in_1, device=LAFs1.device).reshape(-1).long()
    j = torch.as_tensor(tent_in_2, device=LAFs1.device).reshape(-1).long()
    one = torch.ones(i.numel(), 1, dtype=torch.float64, device=LAFs1.device)
    x1 = torch.cat([LAFs1[i][:, :, 2].double(), one], 1)
    x2 = torch.cat([LAFs2.to(LAFs1.device)[j][:, :, 2].double(), one], 1)
    l, m = x1 @ F.t(), x2 @ F                         # F x1, F^T x2
    r = (x2 * l).sum(1)
    return torch.sqrt(r * r / (l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2))


def match_and_verify(descriptors1, descriptors2, LAFs1, LAFs2, SNN_threshold=0.8, inl_th=3.0, model="homography", lo_iters=3, rounds=8, seed=0,
                     matcher="reference", fginn_radius=10.0, mutual=False, plane_th=3.0):
    """match_snn followed by verify_matches as one chain on the stream: the tentative list and its device-side count go from
    affnet_match_snn straight into affnet_verify_matches (model='fundamental': affnet_epipolar_verify, which alone reads `rounds` and
    `seed`; model='fundamental_planar': affnet_epipolar_verify_planar, which reads `plane_th` too and adds verify_epipolar_planar's keys to
    info), and the host reads back once, at the end.
    matcher: 'reference' is affnet_match_snn; 'snn' (the per-row ratio test) and 'fginn' (the ratio against the first neighbour more than
    fginn_radius px from the nearest one) put affnet_match_ratio in its place, with `mutual` as in match_ratio.
    Returns (tent_matches_in_1, tent_matches_in_2, H, inliers (T,) bool, info) - the pieces of match_snn and verify_matches."""
    ratio_radius = _matcher_radius("match_and_verify", matcher, fginn_radius, mutual)
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
    if ratio_radius is not None:
        tent, cnt, _, _ = enqueue_match_ratio(a, b, LAFs2 if ratio_radius >= 0 else None, ratio_radius, SNN_threshold, float("inf"), mutual)
    elif n1:
        md = torch.empty(n1, dtype=torch.float32, device=dev)
        md2 = torch.empty(n1, dtype=torch.float32, device=dev)
        idx = torch.empty(n1, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=dev)
        ctx = engine.utility_ctx(dev)
        rc = lib.affnet_match_snn(ctx, ptr(a), n1, ptr(b), n2, a.size(1), float(SNN_threshold), ptr(md), ptr(idx), ptr(md2), ptr(tent), ptr(cnt),
                                  ptr(scratch), engine.stream_of(dev))
        check(rc, ctx, "affnet_match_snn")
    if model == "fundamental_planar":
        H, inl, counts, summary, Hp, pinl, _, pinfo = enqueue_verify_epipolar_planar(LAFs1, LAFs2, tent, cnt, inl_th, plane_th, rounds, seed, lo_iters)
        host = torch.cat([cnt, summary, pinfo]).cpu().tolist()          # the one read-back
        k = host[0]
        info = dict(_verify_info(counts[:k * int(rounds)], host[1:5]), rounds=int(rounds), seed=int(seed))
        return tent[:k, 0].long(), tent[:k, 1].long(), H, inl[:k].bool(), _planar_info(info, Hp, pinl[:k], host[5])
    if model == "fundamental":
        H, inl, counts, summary = enqueue_verify_epipolar(LAFs1, LAFs2, tent, cnt, inl_th, rounds, seed, lo_iters)
    else:
        H, inl, counts, summary = enqueue_verify(LAFs1, LAFs2, tent, cnt, inl_th, model, lo_iters)
    host = torch.cat([cnt, summary]).cpu().tolist()          # the one read-back
    k = host[0]
    if model == "fundamental":
        return tent[:k, 0].long(), tent[:k, 1].long(), H, inl[:k].bool(), dict(_verify_info(counts[:k * int(rounds)], host[1:]), rounds=int(rounds), seed=int(seed))
    return tent[:k, 0].long(), tent[:k, 1].long(), H, inl[:k].bool(), _verify_info(counts[:k], host[1:])


# ---- many image pairs in one device call (csrc/match.hip affnet_match_snn_many, csrc/spatial.hip affnet_verify_matches_many) ---------------------

def pair_table(counts1, counts2, pairs):
    """Host helper: the (P,4) int32 table {row1, n1, row2, n2} of the *_many calls for `pairs` = [(a, b), ...], image a of side 1 against image b
    of side 2, where image i of a side owns counts[i] consecutive rows of that side's concatenated buffers.
    Returns (table, n1_max, n2_max).  ValueError on an image index out of range (or a negative count)."""
    c1, c2 = [int(c) for c in counts1], [int(c) for c in counts2]
    if any(c < 0 for c in c1 + c2):
        raise ValueError("pair_table: negative row count")
    off1 = np.concatenate([[0], np.cumsum(c1, dtype=np.int64)])
    off2 = np.concatenate([[0], np.cumsum(c2, dtype=np.int64)])
    if max(off1[-1], off2[-1]) > 0x7fffffff:
        raise ValueError("pair_table: more than 2^31 - 1 rows on one side")
    table = np.zeros((len(pairs), 4), np.int32)
    for p, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if not (0 <= a < len(c1) and 0 <= b < len(c2)):
            raise ValueError("pair_table: pair %d = (%d, %d) with %d / %d images" % (p, a, b, len(c1), len(c2)))
        table[p] = (off1[a], c1[a], off2[b], c2[b])
    return table, int(table[:, 1].max()) if len(pairs) else 0, int(table[:, 3].max()) if len(pairs) else 0


def _many_buf(dev, dtype, *shape):
    """Zero-filled device tensor of `shape` whose storage is never empty (the boundary refuses NULL)."""
    n = int(np.prod(shape))
    return torch.zeros(max(n, 1), dtype=dtype, device=dev)[:n].view(*shape)


def _many_model(model, rounds, seed, what):
    """-> (epi, model code or None, rounds, seed, hypotheses per tentative); ValueError on an unknown model or rounds / seed out of range."""
    if model != "fundamental":
        return False, _verify_model(model), int(rounds), int(seed), 1
    rounds, seed = int(rounds), int(seed)
    if not 1 <= rounds <= _lib.EPI_MAX_ROUNDS:
        raise ValueError("%s: rounds must be in 1..%d" % (what, _lib.EPI_MAX_ROUNDS))
    if not 0 <= seed < 2 ** 32:
        raise ValueError("%s: seed must fit 32 unsigned bits" % what)
    return True, None, rounds, seed, rounds


def _many_sides(what, desc1, LAFs1, counts1, desc2, LAFs2, counts2):
    for t, name in ((desc1, "desc1"), (LAFs1, "LAFs1"), (desc2, "desc2"), (LAFs2, "LAFs2")):
        engine.require_cuda(t, name)
    a, b = desc1.contiguous().float(), desc2.contiguous().float()
    l1, l2 = LAFs1.contiguous().float(), LAFs2.contiguous().float()
    rows1, rows2 = a.size(0), b.size(0)
    if l1.size(0) != rows1 or l2.size(0) != rows2:
        raise ValueError("%s: one LAF per descriptor row (%d / %d frames for %d / %d descriptors)" % (what, l1.size(0), l2.size(0), rows1, rows2))
    if sum(int(c) for c in counts1) != rows1 or sum(int(c) for c in counts2) != rows2:
        raise ValueError("%s: the counts do not add up to the rows of the buffers" % what)
    return a, b, l1, l2


class _ManyCall:
    """The buffers that the calls of one *_many chain share, and the calls themselves: every method enqueues on the current stream and returns
    device tensors, nothing synchronises."""

    def __init__(self, a, b, l1, l2, table, cap, n2_max, epi, code, rounds, seed, inl_th, lo_iters):
        self.a, self.b, self.l1, self.l2 = a, b, l1, l2
        self.rows1, self.rows2, self.dev = a.size(0), b.size(0), a.device
        self.P, self.cap, self.n2_max = table.shape[0], cap, n2_max
        self.epi, self.code, self.rounds, self.seed, self.per = epi, code, rounds, seed, rounds if epi else 1
        self.inl_th, self.lo_iters = float(inl_th), int(lo_iters)
        P = self.P
        self.d_pairs = torch.from_numpy(table).to(self.dev)
        verify_bytes = lib.affnet_epipolar_many_scratch_bytes(P, cap, rounds) if epi else lib.affnet_verify_many_scratch_bytes(P, cap)
        self.scratch = torch.empty(max(lib.affnet_match_many_scratch_bytes(P, cap, n2_max), lib.affnet_match_guided_many_scratch_bytes(P, cap, n2_max, 0),
                                       lib.affnet_match_ratio_many_scratch_bytes(P, cap, n2_max, 0), verify_bytes), dtype=torch.uint8, device=self.dev)
        self.one = torch.zeros(8, dtype=torch.float32, device=self.dev)           # stands in for an empty side: never read, but the boundary refuses NULL
        self.ctx, self.st = engine.utility_ctx(self.dev), engine.stream_of(self.dev)

    def _side(self, t, rows):
        return ptr(t if rows else self.one)

    def match(self, SNN_threshold):
        P, cap, dev = self.P, self.cap, self.dev
        tent, cnt = _many_buf(dev, torch.int32, P, cap, 2), _many_buf(dev, torch.int32, P)
        md, md2, idx = _many_buf(dev, torch.float32, P, cap), _many_buf(dev, torch.float32, P, cap), _many_buf(dev, torch.int32, P, cap)
        rc = lib.affnet_match_snn_many(self.ctx, self._side(self.a, self.rows1), self.rows1, self._side(self.b, self.rows2), self.rows2, self.a.size(1),
                                       ptr(self.d_pairs), P, cap, self.n2_max, float(SNN_threshold), ptr(md), ptr(idx), ptr(md2), ptr(tent), ptr(cnt),
                                       ptr(self.scratch), self.st)
        check(rc, self.ctx, "affnet_match_snn_many")
        return tent, cnt

    def match_ratio(self, SNN_threshold, radius, mutual):
        P, cap, dev = self.P, self.cap, self.dev
        tent, cnt = _many_buf(dev, torch.int32, P, cap, 2), _many_buf(dev, torch.int32, P)
        dist, idx = _many_buf(dev, torch.float32, P, cap, 2), _many_buf(dev, torch.int32, P, cap, 2)
        rc = lib.affnet_match_ratio_many(self.ctx, self._side(self.a, self.rows1), self.rows1, self._side(self.b, self.rows2), self.rows2, self.a.size(1),
                                         self._side(self.l2, self.rows2) if radius >= 0 else None, ptr(self.d_pairs), P, cap, self.n2_max, radius,
                                         float(SNN_threshold), float("inf"), _lib.RATIO_MUTUAL if mutual else 0, 0, ptr(dist), ptr(idx), ptr(tent), ptr(cnt),
                                         ptr(self.scratch), self.st)
        check(rc, self.ctx, "affnet_match_ratio_many")
        return tent, cnt

    def verify(self, tent, cnt):
        P, cap, dev = self.P, self.cap, self.dev
        H, inl = _many_buf(dev, torch.float64, P, 3, 3), _many_buf(dev, torch.uint8, P, cap)
        counts, summary = _many_buf(dev, torch.int32, P, cap * self.per), _many_buf(dev, torch.int32, P, 4)
        l1, l2 = self._side(self.l1, self.rows1), self._side(self.l2, self.rows2)
        if self.epi:
            rc = lib.affnet_epipolar_verify_many(self.ctx, l1, self.rows1, l2, self.rows2, ptr(self.d_pairs), P, ptr(tent), ptr(cnt), cap, self.inl_th,
                                                 self.rounds, self.seed, self.lo_iters, ptr(counts), ptr(H), ptr(inl), ptr(summary), ptr(self.scratch), self.st)
            check(rc, self.ctx, "affnet_epipolar_verify_many")
        else:
            rc = lib.affnet_verify_matches_many(self.ctx, l1, self.rows1, l2, self.rows2, ptr(self.d_pairs), P, ptr(tent), ptr(cnt), cap, self.inl_th,
                                                self.code, self.lo_iters, ptr(counts), ptr(H), ptr(inl), ptr(summary), ptr(self.scratch), self.st)
            check(rc, self.ctx, "affnet_verify_matches_many")
        return H, inl, counts, summary

    def guided(self, H, gate, kind, radius, threshold, mutual):
        P, cap, dev = self.P, self.cap, self.dev
        tent, cnt = _many_buf(dev, torch.int32, P, cap, 2), _many_buf(dev, torch.int32, P)
        dist, idx = _many_buf(dev, torch.float32, P, cap, 2), _many_buf(dev, torch.int32, P, cap, 2)
        rc = lib.affnet_match_guided_many(self.ctx, self._side(self.a, self.rows1), self.rows1, self._side(self.b, self.rows2), self.rows2, self.a.size(1),
                                          self._side(self.l1, self.rows1), self._side(self.l2, self.rows2), ptr(self.d_pairs), P, cap, self.n2_max, ptr(H), kind,
                                          radius, float(threshold), float("inf"), _lib.GUIDED_MUTUAL if mutual else 0, 0, ptr(gate), ptr(dist), ptr(idx),
                                          ptr(tent), ptr(cnt), ptr(self.scratch), self.st)
        check(rc, self.ctx, "affnet_match_guided_many")
        return tent, cnt


def enqueue_match_and_verify_many(desc1, LAFs1, counts1, desc2, LAFs2, counts2, pairs, SNN_threshold=0.8, inl_th=3.0, model="homography", lo_iters=3,
                                  rounds=8, seed=0, matcher="reference", fginn_radius=10.0, mutual=False):
    """match_and_verify for P image pairs in one chain of launches on the current stream, no synchronisation.  desc1 (rows1,128) / LAFs1 (rows1,2,3)
    hold the images of side 1 back to back, counts1[i] rows for image i; side 2 likewise (it may be the same tensors); pairs = [(a, b), ...] image
    indices into the two sides.  Returns capacity-sized device tensors, cap = the largest n1 of a pair: (tent (P,cap,2) int32 with indices local to
    the pair's images, count (P,) int32, H (P,3,3) float64, inliers (P,cap) uint8, counts (P,cap) int32, summary (P,4) int32); per pair, rows below
    count[p] are what match_and_verify gives for that pair, bit for bit, rows at or beyond it are zero.
    model='fundamental' verifies with affnet_epipolar_verify_many, which alone reads `rounds` and `seed`: H is then F, and counts is (P, cap*rounds),
    hypothesis h = s * rounds + r of pair p in counts[p, h].
    matcher, fginn_radius, mutual: as in match_and_verify; 'snn' and 'fginn' put affnet_match_ratio_many in the place of affnet_match_snn_many."""
    what = "enqueue_match_and_verify_many"
    ratio_radius = _matcher_radius(what, matcher, fginn_radius, mutual)
    epi, code, rounds, seed, per = _many_model(model, rounds, seed, what)
    a, b, l1, l2 = _many_sides(what, desc1, LAFs1, counts1, desc2, LAFs2, counts2)
    table, cap, n2_max = pair_table(counts1, counts2, pairs)
    P, dev = table.shape[0], a.device
    if P == 0:
        return (_many_buf(dev, torch.int32, P, cap, 2), _many_buf(dev, torch.int32, P), _many_buf(dev, torch.float64, P, 3, 3), _many_buf(dev, torch.uint8, P, cap),
                _many_buf(dev, torch.int32, P, cap * per), _many_buf(dev, torch.int32, P, 4))
    call = _ManyCall(a, b, l1, l2, table, cap, n2_max, epi, code, rounds, seed, inl_th, lo_iters)
    tent, cnt = call.match(SNN_threshold) if ratio_radius is None else call.match_ratio(SNN_threshold, ratio_radius, mutual)
    H, inl, counts, summary = call.verify(tent, cnt)
    return tent, cnt, H, inl, counts, summary


def _many_lists(what, descs, LAFs, pairs):
    """The image lists of the list-taking *_many functions as one (D, L, counts) side, or None for an empty list (with no pairs)."""
    if len(descs) != len(LAFs):
        raise ValueError("%s: one LAF tensor per descriptor tensor" % what)
    for t in list(descs) + list(LAFs):
        engine.require_cuda(t, "descs / LAFs")
    if not len(descs):
        if len(pairs):
            raise ValueError("%s: pairs of an empty image list" % what)
        return None
    counts = [int(d.size(0)) for d in descs]
    if any(int(l.size(0)) != c for l, c in zip(LAFs, counts)):
        raise ValueError("%s: one LAF per descriptor row" % what)
    D = torch.cat([d.contiguous().float() for d in descs], 0)
    L = torch.cat([l.contiguous().float().reshape(-1, 2, 3) for l in LAFs], 0)
    return D, L, counts


def match_and_verify_many(descs, LAFs, pairs, SNN_threshold=0.8, inl_th=3.0, model="homography", lo_iters=3, rounds=8, seed=0, matcher="reference",
                          fginn_radius=10.0, mutual=False):
    """match_and_verify for every pair (a, b) of `pairs`, image indices into the lists descs / LAFs (one (n_i,128) / (n_i,2,3) device tensor per
    image; both sides of a pair come from the same lists), as one device call chain and ONE read-back.  model: 'homography', 'affine' or
    'fundamental' (which alone reads `rounds` and `seed`); matcher, fginn_radius, mutual as in match_and_verify.
    Returns a list of P tuples (tent_matches_in_1, tent_matches_in_2, H, inliers (T,) bool, info), each what match_and_verify returns for that pair."""
    _matcher_radius("match_and_verify_many", matcher, fginn_radius, mutual)
    epi, _, rounds, seed, per = _many_model(model, rounds, seed, "match_and_verify_many")
    side = _many_lists("match_and_verify_many", descs, LAFs, pairs)
    if side is None:
        return []
    D, L, counts = side
    tent, cnt, H, inl, hyp_counts, summary = enqueue_match_and_verify_many(D, L, counts, D, L, counts, pairs, SNN_threshold, inl_th, model, lo_iters, rounds, seed,
                                                                            matcher, fginn_radius, mutual)
    host = torch.cat([cnt.view(-1, 1), summary], 1).cpu().tolist()          # the one read-back
    out = []
    for p, row in enumerate(host):
        k = row[0]
        info = _verify_info(hyp_counts[p, :k * per], row[1:])
        if epi:
            info.update(rounds=rounds, seed=seed)
        out.append((tent[p, :k, 0].long(), tent[p, :k, 1].long(), H[p], inl[p, :k].bool(), info))
    return out


def enqueue_match_verify_guided_many(desc1, LAFs1, counts1, desc2, LAFs2, counts2, pairs, SNN_threshold=0.8, inl_th=3.0, model="homography",
                                     guided_threshold=0.9, radius=None, mutual=True, lo_iters=3, rounds=8, seed=0):
    """match_verify_guided for P image pairs in one chain of launches on the current stream, no synchronisation: affnet_match_snn_many,
    verification, affnet_match_guided_many - which reads row p of the first stage's models as pair p's model and row p of its summaries as pair
    p's gate, on the device - and verification of the guided matches.  Sides, counts and pairs as for enqueue_match_and_verify_many; model:
    'homography', 'affine' or 'fundamental'.
    Returns (tent, count, H, inliers, counts, summary) of the final stage, shaped as enqueue_match_and_verify_many returns them, then count0 (P,)
    int32 and summary0 (P,4) int32 of the first stage."""
    what = "enqueue_match_verify_guided_many"
    if model not in GUIDED_KINDS:
        raise ValueError("model must be 'homography', 'affine' or 'fundamental'")
    kind, radius = _guided_kind(model, radius)
    epi, code, rounds, seed, per = _many_model(model, rounds, seed, what)
    a, b, l1, l2 = _many_sides(what, desc1, LAFs1, counts1, desc2, LAFs2, counts2)
    table, cap, n2_max = pair_table(counts1, counts2, pairs)
    P, dev = table.shape[0], a.device
    if P == 0:
        return (_many_buf(dev, torch.int32, P, cap, 2), _many_buf(dev, torch.int32, P), _many_buf(dev, torch.float64, P, 3, 3), _many_buf(dev, torch.uint8, P, cap),
                _many_buf(dev, torch.int32, P, cap * per), _many_buf(dev, torch.int32, P, 4), _many_buf(dev, torch.int32, P), _many_buf(dev, torch.int32, P, 4))
    call = _ManyCall(a, b, l1, l2, table, cap, n2_max, epi, code, rounds, seed, inl_th, lo_iters)
    tent0, cnt0 = call.match(SNN_threshold)
    H0, _, _, summary0 = call.verify(tent0, cnt0)
    tent, cnt = call.guided(H0, summary0, kind, radius, guided_threshold, mutual)
    H, inl, counts, summary = call.verify(tent, cnt)
    return tent, cnt, H, inl, counts, summary, cnt0, summary0


def match_verify_guided_many(descs, LAFs, pairs, SNN_threshold=0.8, inl_th=3.0, model="homography", guided_threshold=0.9, radius=None, mutual=True,
                             lo_iters=3, rounds=8, seed=0):
    """match_verify_guided for every pair (a, b) of `pairs`, image indices into the lists descs / LAFs as for match_and_verify_many, as one device
    call chain and ONE read-back.  Returns a list of P tuples, each what match_verify_guided returns for that pair, info["seed_stage"] included."""
    if model not in GUIDED_KINDS:
        raise ValueError("model must be 'homography', 'affine' or 'fundamental'")
    epi, _, rounds, seed, per = _many_model(model, rounds, seed, "match_verify_guided_many")
    side = _many_lists("match_verify_guided_many", descs, LAFs, pairs)
    if side is None:
        return []
    D, L, counts = side
    tent, cnt, H, inl, hyp_counts, summary, cnt0, summary0 = enqueue_match_verify_guided_many(D, L, counts, D, L, counts, pairs, SNN_threshold, inl_th, model,
                                                                                              guided_threshold, radius, mutual, lo_iters, rounds, seed)
    host = torch.cat([cnt0.view(-1, 1), summary0, cnt.view(-1, 1), summary], 1).cpu().tolist()          # the one read-back
    out = []
    for p, row in enumerate(host):
        k = row[5]
        info = _verify_info(hyp_counts[p, :k * per], row[6:])
        if epi:
            info.update(rounds=rounds, seed=seed)
        info["seed_stage"] = {"tentatives": row[0], "num_inliers": row[3], "flags": row[4]}
        out.append((tent[p, :k, 0].long(), tent[p, :k, 1].long(), H[p], inl[p, :k].bool(), info))
    return out


def spatial_rerank(descs, LAFs, query, shortlist, SNN_threshold=0.8, inl_th=3.0, model="homography", lo_iters=3, rounds=8, seed=0, guided=False,
                   matcher="reference", fginn_radius=10.0, mutual=False):
    """Re-ranks `shortlist` (image indices into descs / LAFs) by the number of verified inliers against image `query`, all pairs in one device call
    chain.  model: 'homography', 'affine' or 'fundamental' (a scene with depth; it alone reads `rounds` and `seed`); guided: the inliers of
    match_verify_guided_many (defaults of its guided_threshold and radius) instead of match_and_verify_many's.  matcher, fginn_radius, mutual: the
    first stage of the unguided chain, as in match_and_verify.
    Returns (order, num_inliers): the shortlist sorted by descending inlier count, ties in shortlist order, and the counts in that order."""
    _matcher_radius("spatial_rerank", matcher, fginn_radius, mutual, guided)
    shortlist = [int(s) for s in shortlist]
    pairs = [(int(query), s) for s in shortlist]
    if guided:
        res = match_verify_guided_many(descs, LAFs, pairs, SNN_threshold, inl_th, model, lo_iters=lo_iters, rounds=rounds, seed=seed)
    else:
        res = match_and_verify_many(descs, LAFs, pairs, SNN_threshold, inl_th, model, lo_iters, rounds, seed, matcher, fginn_radius, mutual)
    n = [r[4]["num_inliers"] for r in res]
    rank = sorted(range(len(shortlist)), key=lambda i: -n[i])          # sorted() is stable: ties keep the shortlist's order
    return [shortlist[i] for i in rank], [n[i] for i in rank]


# ---- guided matching (csrc/guided.hip: affnet_match_guided, affnet_guided_mask) ----------------------------------------------------------------

GUIDED_KINDS = {"homography": _lib.GUIDED_PLANAR, "affine": _lib.GUIDED_PLANAR, "fundamental": _lib.GUIDED_EPIPOLAR}
GUIDED_RADIUS = {_lib.GUIDED_PLANAR: 10.0, _lib.GUIDED_EPIPOLAR: 4.0}          # px: the default search radius of a model family


def _guided_kind(kind, radius):
    if kind not in GUIDED_KINDS:
        raise ValueError("kind must be 'homography', 'affine' or 'fundamental'")
    code = GUIDED_KINDS[kind]
    return code, float(GUIDED_RADIUS[code] if radius is None else radius)


def _guided_model(model, dev):
    """(3,3) float64 on `dev`: a device tensor is read where it lies, a host value is uploaded."""
    m = model if torch.is_tensor(model) else torch.as_tensor(np.asarray(model, np.float64))
    if m.numel() != 9:
        raise ValueError("model must have 9 entries")
    return m.to(device=dev, dtype=torch.float64).contiguous()


def _guided_frames(what, desc1, desc2, LAFs1, LAFs2):
    for t, name in ((desc1, "desc1"), (desc2, "desc2"), (LAFs1, "LAFs1"), (LAFs2, "LAFs2")):
        engine.require_cuda(t, name)
    a, b = desc1.contiguous().float(), desc2.contiguous().float()
    if b.size(0) == 0:
        raise ValueError("%s: descriptors2 is empty" % what)
    if LAFs1.size(0) != a.size(0) or LAFs2.size(0) != b.size(0):
        raise ValueError("%s: one LAF per descriptor row (%d / %d frames for %d / %d descriptors)" % (what, LAFs1.size(0), LAFs2.size(0), a.size(0), b.size(0)))
    return a, b, LAFs1.contiguous().float(), LAFs2.contiguous().float()


def enqueue_match_guided(desc1, desc2, LAFs1, LAFs2, model, kind="homography", radius=None, SNN_threshold=0.9, max_dist=float("inf"), mutual=True,
                         gate=None, n_chunks=0):
    """Guided matching (affnet_match_guided) enqueued on the current stream with no synchronisation: every row of desc1 is matched among the rows
    of desc2 whose frame centre the model allows - within `radius` px of where a 'homography' / 'affine' model (3,3 map of image 1 to image 2)
    sends the row's centre, or within `radius` px (Sampson) of its epipolar line under a 'fundamental' model.  model: (3,3) float64, a device
    tensor as a verification call returns it (read in place) or a host value (uploaded).  radius: default 10 px planar, 4 px 'fundamental'.
    A pair is kept when its distance is <= max_dist, its ratio to the second admissible neighbour is <= SNN_threshold and, with `mutual`, the
    row is also the nearest admissible row of its column.  gate: the (4,) int32 summary of a verification call, or None; when its flags say
    "no valid hypothesis" nothing is matched.
    Returns capacity-sized device tensors (tent (n1,2) int32, count (1,) int32, dist (n1,2), idx (n1,2) int32: the two nearest admissible columns
    per row, (+inf, -1) where there is none); rows of tent at or beyond the count are zero."""
    a, b, l1, l2 = _guided_frames("enqueue_match_guided", desc1, desc2, LAFs1, LAFs2)
    code, radius = _guided_kind(kind, radius)
    n1, n2, dev = a.size(0), b.size(0), a.device
    if gate is not None and (gate.dtype != torch.int32 or gate.numel() != 4 or not gate.is_cuda):
        raise ValueError("enqueue_match_guided: gate must be a (4,) int32 device tensor or None")
    m = _guided_model(model, dev)
    tent = torch.zeros(max(n1, 1), 2, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    dist = torch.full((max(n1, 1), 2), float("inf"), dtype=torch.float32, device=dev)
    idx = torch.full((max(n1, 1), 2), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.affnet_match_guided_scratch_bytes(n1, n2, int(n_chunks)), dtype=torch.uint8, device=dev)
    one = torch.zeros(8, dtype=torch.float32, device=dev)           # stands in for an empty side: never read, but the boundary refuses NULL
    ctx = engine.utility_ctx(dev)
    rc = lib.affnet_match_guided(ctx, ptr(a if n1 else one), n1, ptr(b), n2, a.size(1), ptr(l1 if n1 else one), ptr(l2), ptr(m), code, radius,
                                 float(SNN_threshold), float(max_dist), _lib.GUIDED_MUTUAL if mutual else 0, int(n_chunks), ptr(gate), ptr(dist), ptr(idx),
                                 ptr(tent), ptr(cnt), ptr(scratch), engine.stream_of(dev))
    check(rc, ctx, "affnet_match_guided")
    return tent[:n1], cnt, dist[:n1], idx[:n1]


def match_guided(desc1, desc2, LAFs1, LAFs2, model, kind="homography", radius=None, SNN_threshold=0.9, max_dist=float("inf"), mutual=True, gate=None,
                 n_chunks=0):
    """enqueue_match_guided and one read-back.  Returns (tent_matches_in_1, tent_matches_in_2, dist (n1,2), idx (n1,2)) - the first two int64, as
    match_snn returns them."""
    tent, cnt, dist, idx = enqueue_match_guided(desc1, desc2, LAFs1, LAFs2, model, kind, radius, SNN_threshold, max_dist, mutual, gate, n_chunks)
    k = int(cnt.item())
    return tent[:k, 0].long(), tent[:k, 1].long(), dist, idx


def guided_mask(LAFs1, LAFs2, model, kind="homography", radius=None):
    """(n1,n2) bool: the pairs of frames that guided matching under this model, kind and radius admits (affnet_guided_mask)."""
    engine.require_cuda(LAFs1, "LAFs1")
    engine.require_cuda(LAFs2, "LAFs2")
    code, radius = _guided_kind(kind, radius)
    l1, l2 = LAFs1.contiguous().float(), LAFs2.contiguous().float()
    n1, n2, dev = l1.size(0), l2.size(0), l1.device
    mask = torch.zeros(max(n1 * n2, 1), dtype=torch.uint8, device=dev)
    if n1 and n2:
        m = _guided_model(model, dev)
        scratch = torch.empty(lib.affnet_match_guided_scratch_bytes(n1, n2, 1), dtype=torch.uint8, device=dev)
        ctx = engine.utility_ctx(dev)
        check(lib.affnet_guided_mask(ctx, ptr(l1), n1, ptr(l2), n2, ptr(m), code, radius, ptr(mask), ptr(scratch), engine.stream_of(dev)), ctx,
              "affnet_guided_mask")
    return mask[:n1 * n2].view(n1, n2).bool()


def match_verify_guided(descriptors1, descriptors2, LAFs1, LAFs2, SNN_threshold=0.8, inl_th=3.0, model="homography", guided_threshold=0.9, radius=None,
                        mutual=True, lo_iters=3, rounds=8, seed=0, plane_th=3.0):
    """match_snn, verification, guided matching under the verified model, verification of the guided matches - one chain on the stream: the
    tentative lists, their device-side counts, the first model and its summary (the guided call's gate) pass from call to call on the device,
    and the host reads back once, at the end.  model: 'homography', 'affine', 'fundamental' or 'fundamental_planar' (both stages verify with
    affnet_epipolar_verify_planar, the guided stage reads its F as kind 'fundamental'), as in match_and_verify.
    Returns match_and_verify's tuple for the final stage: (tent_matches_in_1, tent_matches_in_2, H, inliers (T,) bool, info), with
    info["seed_stage"] = {tentatives, num_inliers, flags} of the first stage.  When the first stage found no model (its flags & 1) the final
    lists are empty and the final flags say so too."""
    a, b, l1, l2 = _guided_frames("match_verify_guided", descriptors1, descriptors2, LAFs1, LAFs2)
    planar = model == "fundamental_planar"
    if planar:
        model = "fundamental"
    if model not in GUIDED_KINDS:
        raise ValueError("model must be 'homography', 'affine', 'fundamental' or 'fundamental_planar'")
    n1, n2, dev = a.size(0), b.size(0), a.device
    epi = model == "fundamental"

    def verify(tent, cnt):
        if planar:
            return enqueue_verify_epipolar_planar(l1, l2, tent, cnt, inl_th, plane_th, rounds, seed, lo_iters)
        if epi:
            return enqueue_verify_epipolar(l1, l2, tent, cnt, inl_th, rounds, seed, lo_iters)
        return enqueue_verify(l1, l2, tent, cnt, inl_th, model, lo_iters)

    tent0 = torch.empty(n1, 2, dtype=torch.int32, device=dev)
    cnt0 = torch.zeros(1, dtype=torch.int32, device=dev)
    if n1:
        md = torch.empty(n1, dtype=torch.float32, device=dev)
        md2 = torch.empty(n1, dtype=torch.float32, device=dev)
        idx = torch.empty(n1, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=dev)
        ctx = engine.utility_ctx(dev)
        rc = lib.affnet_match_snn(ctx, ptr(a), n1, ptr(b), n2, a.size(1), float(SNN_threshold), ptr(md), ptr(idx), ptr(md2), ptr(tent0), ptr(cnt0),
                                  ptr(scratch), engine.stream_of(dev))
        check(rc, ctx, "affnet_match_snn")
    H0, _, _, summary0 = verify(tent0, cnt0)[:4]
    tent, cnt, _, _ = enqueue_match_guided(a, b, l1, l2, H0, model, radius, guided_threshold, float("inf"), mutual, summary0)
    tent = tent.contiguous()
    final = verify(tent, cnt)
    H, inl, counts, summary = final[:4]
    host = torch.cat([cnt0, summary0, cnt, summary] + ([final[7]] if planar else [])).cpu().tolist()          # the one read-back
    k = host[5]
    per = int(rounds) if epi else 1
    info = _verify_info(counts[:k * per], host[6:10])
    if epi:
        info.update(rounds=int(rounds), seed=int(seed))
    if planar:
        _planar_info(info, final[4], final[5][:k], host[10])
    info["seed_stage"] = {"tentatives": host[0], "num_inliers": host[3], "flags": host[4]}
    return tent[:k, 0].long(), tent[:k, 1].long(), H, inl[:k].bool(), info
