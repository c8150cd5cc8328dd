#!/usr/bin/env python
"""graf 1 <-> 6 matching check = test() of the reference (train_AffNet_test_on_graffity.py:262-339), on the MI355X:
detect + AffNet + OriNet + HardNet on both images (one batched call when they have the same size), SNN ratio matching
(MFMA distance kernel, no N x N matrix in HBM), homography consistency at 6 px.

    python examples/graf_matching/match_graf.py [--desc hardnet|sift|tfeat] [--tfeat-weights PATH] [--verify [--model homography|fundamental|fundamental_planar] [--guided]]
                                                 [--matcher reference|snn|fginn [--mutual] [--fginn-radius R]] [IMG1 IMG2 H1to2 [N [HARDNET.pth]]]

Defaults: tests/golden/graf_img1.png, graf_img6.png, graf_H1to6p, N = 3000, --desc hardnet.  The reference's HardNet++.pth is a
missing blob; without a checkpoint the seeded synthetic HardNet is used, whose descriptors are not discriminative (few matches).
--desc sift: SIFTNet(patch_size=32), the descriptor the reference's test() constructs (train_AffNet_test_on_graffity.py:122) - no
weights needed; at N = 500 it gives the reference's 79 tentatives / 4 true matches.
--desc tfeat: HardTFeatNet (HardNet.py:30-59), the reference's `--descriptor TFeat`.  --tfeat-weights: a .pth with a `state_dict` (the
reference's HardTFeat.pth) or one of the fixtures tests/golden/tfeat_weights_{0,1,2}.npz (the three are read together); default: the
fixtures.  With the trained weights at N = 500 the reference gives 34 tentatives / 5 true matches.
--verify: matching and geometric verification WITHOUT the ground truth in one device chain (match_and_verify: every tentative's pair of affine
frames is an affine hypothesis, all scored against all, the best refined as a homography); a second line per run gives the inlier count, how
many of the inliers the ground-truth homography confirms (the same 6 px centre rule) and how far the recovered H moves the image corners from
where the file's H puts them.
--model fundamental (with --verify): the epipolar model instead (model="fundamental": three tentatives' frames give one 8-point hypothesis, the
best refined as a rank-2 fundamental matrix, Sampson error <= 2 px); the line gives the epipolar inliers next to the ground-truth check and the
median Sampson distance of the ground-truth matches under the recovered F.  graf is a PLANAR scene: every F compatible with its homography
explains the wall, so the F printed here is one of a family - good as an inlier test, not as the pair's epipolar geometry.  The model is
meant for two views of a scene with depth, where a homography keeps only the dominant plane.
--model fundamental_planar (with --verify): the plane-aware epipolar model (verify_epipolar_planar: the dominant plane's homography first, then
F = [e]x H from the matches off that plane, kept when it has more inliers than the 8-point F); the line says which of the two models was kept,
how many matches lie off the plane and how many inliers the plane has.  On graf, a wall, there is next to nothing off the plane: the 8-point
model is expected to stay.
--guided (with --verify): guided matching behind the verification (match_verify_guided: the descriptors are searched again, every keypoint among
the keypoints the verified model allows, and the result is verified once more); a further line gives the guided tentatives, their verified
inliers and how many of each the ground-truth homography confirms, by the same 6 px rule.
--matcher: the matcher in front of everything else.  reference (the default) is the evaluation script's (match_snn: the second minimum runs over
the columns that are nobody's nearest neighbour); snn is the per-row ratio test (match_ratio); fginn takes the ratio against the nearest
descriptor whose centre lies more than --fginn-radius px (default 10) from the nearest neighbour's (match_fginn), so that a second detection of
the same structure does not refuse a good match.  --mutual (snn, fginn): keep a match only if it is also the nearest one backwards.  --verify
passes the choice to match_and_verify; --guided keeps the reference matcher as its first stage and goes with it only."""
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import affnet_amd  # noqa: E402
from affnet_amd.ReprojectionStuff import match_snn, match_ratio, match_and_verify, match_verify_guided, get_GT_correspondence_indexes, sampson_distance  # noqa: E402


def load_grayscale_var(fname):        # train_AffNet_test_on_graffity.py:246-253
    img = np.mean(np.array(Image.open(fname).convert("RGB")), axis=2)
    return torch.from_numpy(img.astype(np.float32)).view(1, 1, img.shape[0], img.shape[1])


def load_tfeat_state(path):
    """A .pth checkpoint with `state_dict`, or the weight fixtures (any of the three .npz names, or None): the six tensors by their reference names."""
    if path and path.endswith(".pth"):
        return torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
    gd = os.path.dirname(os.path.abspath(path)) if path else os.path.join(ROOT, "tests", "golden")
    parts = [np.load(os.path.join(gd, "tfeat_weights_%d.npz" % i)) for i in range(3)]
    sd = {k: torch.from_numpy(parts[0][k]) for k in affnet_amd.HardTFeatNet.KEYS[:4]}
    sd["classifier.1.weight"] = torch.from_numpy(np.concatenate([p["classifier.1.weight.part"] for p in parts], 0))
    sd["classifier.1.bias"] = torch.from_numpy(parts[2]["classifier.1.bias"])
    return sd


def main(argv):
    desc_kind = "hardnet"
    tfeat_path = None
    verify = "--verify" in argv
    guided = "--guided" in argv
    if guided and not verify:
        sys.exit("--guided goes with --verify")
    mutual = "--mutual" in argv
    argv = [a for a in argv if a not in ("--verify", "--guided", "--mutual")]
    matcher, fginn_radius = "reference", 10.0
    if "--matcher" in argv:
        i = argv.index("--matcher")
        if i + 1 >= len(argv) or argv[i + 1] not in ("reference", "snn", "fginn"):
            sys.exit("--matcher takes reference, snn or fginn")
        matcher = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if "--fginn-radius" in argv:
        i = argv.index("--fginn-radius")
        try:
            fginn_radius = float(argv[i + 1])
        except (IndexError, ValueError):
            sys.exit("--fginn-radius takes a number of pixels")
        if not 0 <= fginn_radius < float("inf"):
            sys.exit("--fginn-radius takes a finite number >= 0")
        argv = argv[:i] + argv[i + 2:]
    if matcher == "reference" and mutual:
        sys.exit("--mutual goes with --matcher snn or fginn")
    if matcher != "reference" and guided:
        sys.exit("--guided keeps the reference matcher as its first stage: it goes with --matcher reference")
    mkw = {} if matcher == "reference" else dict(matcher=matcher, fginn_radius=fginn_radius, mutual=mutual)
    mtag = "" if matcher == "reference" else " [%s%s%s]" % (matcher, " radius %g" % fginn_radius if matcher == "fginn" else "", " mutual" if mutual else "")
    if "--tfeat-weights" in argv:
        i = argv.index("--tfeat-weights")
        if i + 1 >= len(argv):
            sys.exit("--tfeat-weights takes a path")
        tfeat_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    model = "homography"
    if "--model" in argv:
        i = argv.index("--model")
        if i + 1 >= len(argv) or argv[i + 1] not in ("homography", "fundamental", "fundamental_planar"):
            sys.exit("--model takes homography, fundamental or fundamental_planar")
        model = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if "--desc" in argv:
        i = argv.index("--desc")
        if i + 1 >= len(argv) or argv[i + 1] not in ("hardnet", "sift", "tfeat"):
            sys.exit("--desc takes hardnet, sift or tfeat")
        desc_kind = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    gd = os.path.join(ROOT, "tests", "golden")
    f1, f2, fh = (argv + [None] * 3)[:3]
    f1, f2, fh = f1 or os.path.join(gd, "graf_img1.png"), f2 or os.path.join(gd, "graf_img6.png"), fh or os.path.join(gd, "graf_H1to6p")
    n = int(argv[3]) if len(argv) > 3 else 3000
    dev = torch.device("cuda:0")
    ld = lambda p: torch.load(p, map_location="cpu", weights_only=False)["state_dict"]
    A = affnet_amd.AffNetFast(PS=32); A.load_state_dict(ld(os.path.join(ROOT, "pretrained", "AffNet.pth")))
    O = affnet_amd.OriNetFast(PS=32); O.load_state_dict(ld(os.path.join(ROOT, "pretrained", "OriNet.pth")))
    Hn = affnet_amd.HardNet(); Hn.load_state_dict(ld(argv[4]) if len(argv) > 4 else affnet_amd.synthetic_hardnet_state(0))
    A, O, Hn = A.to(dev), O.to(dev), Hn.to(dev)
    desc = affnet_amd.SIFTNet(patch_size=32) if desc_kind == "sift" else Hn
    if desc_kind == "tfeat":
        desc = affnet_amd.HardTFeatNet(sm=affnet_amd.SIFTNet(patch_size=32))
        desc.load_state_dict(load_tfeat_state(tfeat_path))
        desc = desc.to(dev)
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=n, border=5, num_Baum_iters=1, AffNet=A, OriNet=O).to(dev)
    img1, img2 = load_grayscale_var(f1).to(dev), load_grayscale_var(f2).to(dev)
    H1to2 = torch.from_numpy(np.loadtxt(fh)).float()
    for do_ori, tag in ((True, "graf1-6"), (False, "ori graf1-6")):
        if img1.shape == img2.shape:
            r1, r2 = det.run_batch(torch.cat([img1, img2], 0), do_ori=do_ori, desc=desc)
        else:
            r1, r2 = det.run(img1, do_ori=do_ori, desc=desc), det.run(img2, do_ori=do_ori, desc=desc)
        if matcher == "reference":
            t1, t2, _, _ = match_snn(r1["descriptors"], r2["descriptors"], 0.8)
        else:
            t1, t2, _, _ = match_ratio(r1["descriptors"], r2["descriptors"], r2["LAFs"], fginn_radius if matcher == "fginn" else None, 0.8, mutual=mutual)
        _, plain, _ = get_GT_correspondence_indexes(r1["LAFs"][t1], r2["LAFs"][t2], H1to2, dist_threshold=6)
        print("Test on %s%s, %d tentatives %d true matches %s  inl.ratio" % (tag, mtag, t1.numel(), plain.numel(), str(plain.numel() / max(1, t1.numel()))[:5]))
        if verify and model in ("fundamental", "fundamental_planar"):
            v1, v2, F, inl, info = match_and_verify(r1["descriptors"], r2["descriptors"], r1["LAFs"], r2["LAFs"], 0.8, inl_th=2.0, model=model, **mkw)
            assert torch.equal(v1, t1) and torch.equal(v2, t2)
            _, ok, _ = get_GT_correspondence_indexes(r1["LAFs"][v1[inl]], r2["LAFs"][v2[inl]], H1to2, dist_threshold=6)
            d = sampson_distance(F, r1["LAFs"], r2["LAFs"], t1[plain], t2[plain])
            print("Verified on %s (fundamental; planar scene: F is one of a family), %d epipolar inliers of %d tentatives (best hypothesis %d, flags %d), %d of them "
                  "true matches, median Sampson distance of the %d true matches %.2f px"
                  % (tag, info["num_inliers"], v1.numel(), info["best_count"], info["flags"], ok.numel(), plain.numel(), d.median().item() if d.numel() else float("nan")))
            if model == "fundamental_planar":
                print("Plane-aware on %s: kept the %s model; plane with %d inliers, %d matches off the plane"
                      % (tag, "plane-and-parallax" if info["planar"] else "8-point", int(info["plane_inliers"].sum()), info["n_off_plane"]))
        elif verify:
            v1, v2, H, inl, info = match_and_verify(r1["descriptors"], r2["descriptors"], r1["LAFs"], r2["LAFs"], 0.8, inl_th=3.0, **mkw)
            assert torch.equal(v1, t1) and torch.equal(v2, t2)
            _, ok, _ = get_GT_correspondence_indexes(r1["LAFs"][v1[inl]], r2["LAFs"][v2[inl]], H1to2, dist_threshold=6)
            h, w = img1.shape[2], img1.shape[3]
            c = torch.tensor([[0.0, 0.0, 1.0], [w, 0.0, 1.0], [w, h, 1.0], [0.0, h, 1.0]], dtype=torch.float64)
            a, b = c @ H.cpu().T, c @ H1to2.double().T
            err = ((a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]) ** 2).sum(1).sqrt().max().item()
            print("Verified on %s, %d inliers of %d tentatives (best hypothesis %d, flags %d), %d of them true matches, corner error vs H1to2 %.1f px"
                  % (tag, info["num_inliers"], v1.numel(), info["best_count"], info["flags"], ok.numel(), err))
        if verify and guided:
            g1, g2, _, ginl, ginfo = match_verify_guided(r1["descriptors"], r2["descriptors"], r1["LAFs"], r2["LAFs"], 0.8, inl_th=3.0 if model == "homography" else 2.0,
                                                         model=model)
            gt = lambda a, b: get_GT_correspondence_indexes(r1["LAFs"][a], r2["LAFs"][b], H1to2, dist_threshold=6)[1].numel() if a.numel() else 0
            print("Guided on %s (%s), %d guided tentatives %d true matches, %d inliers (flags %d, seed stage flags %d), %d of them true matches"
                  % (tag, model, g1.numel(), gt(g1, g2), ginfo["num_inliers"], ginfo["flags"], ginfo["seed_stage"]["flags"], gt(g1[ginl], g2[ginl])))


if __name__ == "__main__":
    main(sys.argv[1:])
