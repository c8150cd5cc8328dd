#!/usr/bin/env python
"""Retrieval of one query image from a set of images: descriptor index -> vote shortlist -> spatial verification, on the MI355X.

    python examples/graf_matching/retrieve.py [--n N] [--top K] [--k K] [--desc hardnet|sift] [--hardnet HARDNET.pth] [--q8] [--ivf [--cells N --nprobe P]] [--model homography|affine|fundamental] [--guided] [--matcher reference|snn|fginn] QUERY IMG [IMG ...]

Every image goes through the fused path (detect + AffNet + OriNet + descriptor, N = 1000 keypoints by default).  The IMGs become one
DescriptorIndex; the query's descriptors are searched against all of them at once (affnet_knn, --k neighbours per descriptor, default 4), every image
collects the votes of the neighbours that stand out from the background (affnet_knn_vote), and the --top (default 10) images with the most votes
are matched and verified from their affine frames in one device call (affnet_match_snn_many / affnet_verify_matches_many).  Prints the vote
shortlist and the verified order.  Without a HardNet checkpoint the seeded synthetic HardNet is used, whose descriptors are not discriminative;
--desc sift needs no weights.  --q8 builds a QuantizedDescriptorIndex instead: the search runs on int8 descriptors
(affnet_quantize_desc, affnet_knn_q8), the matching and verification of the shortlist on the float ones as before.  --ivf builds an IVFDescriptorIndex: a k-means codebook of --cells
cells (default: the power of two nearest the square root of the number of descriptors) is trained on the index's descriptors, and every query descriptor
is compared with the descriptors of its --nprobe (default 8, at most 8) nearest cells only (affnet_ivf_search).  --q8 --ivf together build
an IVFQuantizedDescriptorIndex: the same codebook, the cells hold the int8 rows (affnet_ivf_search_q8).  --model fundamental verifies the shortlist
with the epipolar model of a scene with depth (affnet_epipolar_verify_many); --guided re-matches every shortlisted image under its verified model
and verifies again (affnet_match_guided_many), still in one chain with one read-back.  --matcher snn / fginn matches the shortlist with
the per-row ratio test / the first geometrically inconsistent neighbour at 10 px (affnet_match_ratio_many) instead of the reference's matcher (not
with --guided, whose first stage stays).  A demonstration of the calls, not a retrieval-quality claim.

    python examples/graf_matching/retrieve.py --desc sift tests/golden/graf_img1.png tests/golden/graf_img6.png tests/golden/graf_img1.png"""
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
    top, argv = take(argv, "--top", "10")
    k, argv = take(argv, "--k", "4")
    desc_kind, argv = take(argv, "--desc", "hardnet")
    hardnet_path, argv = take(argv, "--hardnet", None)
    cells, argv = take(argv, "--cells", None)
    nprobe, argv = take(argv, "--nprobe", "8")
    model, argv = take(argv, "--model", "homography")
    matcher, argv = take(argv, "--matcher", "reference")
    q8, ivf, guided = "--q8" in argv, "--ivf" in argv, "--guided" in argv
    argv = [a for a in argv if a not in ("--q8", "--ivf", "--guided")]
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
    names = argv[1:]
    if ivf:
        index = (affnet_amd.IVFQuantizedDescriptorIndex if q8 else affnet_amd.IVFDescriptorIndex)(descs[1:], lafs[1:], n_cells=int(cells) if cells else None,
                                                                                                  nprobe=int(nprobe))
        print("inverted file: %d cells, %d probed per descriptor" % (index.n_cells, index.nprobe))
    else:
        index = (affnet_amd.QuantizedDescriptorIndex if q8 else affnet_amd.DescriptorIndex)(descs[1:], lafs[1:])
    if q8:
        print("int8 index: scale %.4f" % index.scale)
    print("query %s: %d keypoints against %d images, %d descriptors in the index" % (argv[0], descs[0].size(0), len(index), index.D.size(0)))
    images, votes = index.shortlist(descs[0], top=int(top), k=int(k))
    print("vote shortlist (k = %d):" % int(k))
    for rank, (i, v) in enumerate(zip(images, votes)):
        print("%2d. %s  %d votes (%d keypoints)" % (rank + 1, names[i], v, index.counts[i]))
    print("verified order (model %s%s%s):" % (model, ", guided" if guided else "", ", matcher " + matcher if matcher != "reference" else ""))
    for rank, r in enumerate(index.retrieve(descs[0], lafs[0], top=int(top), k=int(k), SNN_threshold=0.8, inl_th=3.0, model=model, guided=guided, matcher=matcher)):
        first = " (first stage: %d inliers of %d tentatives)" % (r["seed_stage"]["num_inliers"], r["seed_stage"]["tentatives"]) if guided else ""
        print("%2d. %s  %d verified inliers of %d tentatives (%d votes)%s" % (rank + 1, names[r["image"]], r["num_inliers"], r["tent_in_1"].numel(), r["votes"], first))


if __name__ == "__main__":
    main(sys.argv[1:])
