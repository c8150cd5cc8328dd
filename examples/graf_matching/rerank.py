#!/usr/bin/env python
"""Spatial re-ranking of a shortlist: one query image against K images, matched and verified in one device call, on the MI355X.

    python examples/graf_matching/rerank.py [--n N] [--desc hardnet|sift] [--hardnet HARDNET.pth] [--model homography|affine|fundamental] [--guided] [--matcher reference|snn|fginn] QUERY IMG [IMG ...]

Every image goes through the fused path (detect + AffNet + OriNet + descriptor, N = 1000 keypoints by default), then
spatial_rerank(descs, LAFs, 0, [1 .. K]): SNN matching and verification of all K pairs from their affine frames as ONE chain of launches
(affnet_match_snn_many / affnet_verify_matches_many) with one read-back.  Prints the shortlist by descending number of verified inliers
(ties in the order given).  Without a HardNet checkpoint the seeded synthetic HardNet is used, whose descriptors are not discriminative;
--desc sift needs no weights.  --model fundamental verifies with the epipolar model of a scene with depth (affnet_epipolar_verify_many); --guided
re-matches every pair under its verified model and verifies again (affnet_match_guided_many), still one chain and one read-back.  --matcher snn / fginn
puts the per-row ratio test / the first geometrically inconsistent neighbour at 10 px (affnet_match_ratio_many) in the place of the reference's
matcher (not with --guided, whose first stage stays).  A
demonstration of the call, not a retrieval-quality claim.

    python examples/graf_matching/rerank.py tests/golden/graf_img1.png tests/golden/graf_img6.png tests/golden/graf_img1.png"""
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import affnet_amd  # noqa: E402


def load_grayscale_var(fname):        # train_AffNet_test_on_graffity.py:246-253
    img = np.mean(np.array(Image.open(fname).convert("RGB")), axis=2)
    return torch.from_numpy(img.astype(np.float32)).view(1, 1, img.shape[0], img.shape[1])


def take(argv, flag, default):
    if flag not in argv:
        return default, argv
    i = argv.index(flag)
    if i + 1 >= len(argv):
        sys.exit(flag + " takes a value")
    return argv[i + 1], argv[:i] + argv[i + 2:]


def main(argv):
    n, argv = take(argv, "--n", "1000")
    desc_kind, argv = take(argv, "--desc", "hardnet")
    hardnet_path, argv = take(argv, "--hardnet", None)
    model, argv = take(argv, "--model", "homography")
    matcher, argv = take(argv, "--matcher", "reference")
    guided = "--guided" in argv
    argv = [a for a in argv if a != "--guided"]
    if desc_kind not in ("hardnet", "sift") or model not in ("homography", "affine", "fundamental") or matcher not in ("reference", "snn", "fginn") or \
            (guided and matcher != "reference") or len(argv) < 2:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    ld = lambda p: torch.load(p, map_location="cpu", weights_only=False)["state_dict"]
    A = affnet_amd.AffNetFast(PS=32); A.load_state_dict(ld(os.path.join(ROOT, "pretrained", "AffNet.pth")))
    O = affnet_amd.OriNetFast(PS=32); O.load_state_dict(ld(os.path.join(ROOT, "pretrained", "OriNet.pth")))
    if desc_kind == "sift":
        desc = affnet_amd.SIFTNet(patch_size=32)
    else:
        desc = affnet_amd.HardNet()
        desc.load_state_dict(ld(hardnet_path) if hardnet_path else affnet_amd.synthetic_hardnet_state(0))
        desc = desc.to(dev)
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=int(n), border=5, num_Baum_iters=1, AffNet=A.to(dev), OriNet=O.to(dev)).to(dev)
    descs, lafs = [], []
    for f in argv:
        r = det.run(load_grayscale_var(f).to(dev), do_ori=True, desc=desc)
        descs.append(r["descriptors"])
        lafs.append(r["LAFs"])
    shortlist = list(range(1, len(argv)))
    order, num = affnet_amd.spatial_rerank(descs, lafs, 0, shortlist, SNN_threshold=0.8, inl_th=3.0, model=model, guided=guided, matcher=matcher)
    print("query %s: %d keypoints; %d pairs in one device call chain (model %s%s%s)" % (argv[0], descs[0].size(0), len(shortlist), model, ", guided" if guided else "",
                                                                                        ", matcher " + matcher if matcher != "reference" else ""))
    for rank, (i, k) in enumerate(zip(order, num)):
        print("%2d. %s  %d verified inliers (%d keypoints, shortlist position %d)" % (rank + 1, argv[i], k, descs[i].size(0), i))


if __name__ == "__main__":
    main(sys.argv[1:])
