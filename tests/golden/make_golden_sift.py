"""Golden vectors for the SIFT descriptor: the UNMODIFIED reference SIFTNet(patch_size=32)
(pytorch_sift.py:30-94) on CPU, loaded where it lies through oracle/ref_harness.py, and the matching steps of
train_AffNet_test_on_graffity.py:292-305 on its descriptors (the reference's own distance_matrix_vector and
get_GT_correspondence_indexes; the nearest / second-nearest ratio test restated on their results).

    python tests/golden/make_golden_sift.py          -> tests/golden/sift_graf16_n500.npz

Inputs: graf img1 / img6, 500 keypoints each (mrSize 5.192, border 5, the shipped AffNet and OriNet, do_ori), 32 x 32 patches from
extract_patches_from_pyr; twelve synthetic edge-case patches.  Runs only where the reference is available; nothing of it is copied."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402
from make_golden import load_gray  # noqa: E402
from _sift_fp64 import sift_fp64  # noqa: E402

N_PATCHES = 32         # patches stored per image (their descriptors are rows [:32] of desc1 / desc2)
SNN = 0.8
NEAR = 5e-3            # |ratio - SNN| below which a tentative is "borderline" for the GPU matching test


def edge_patches():
    """(12,32,32): all zero, all 255, four uniform-noise patches (seeds 0..3), horizontal ramp, vertical ramp, and four single
    bright pixels (255 on zero) at (0,0), (31,31), (28,28), (29,29)."""
    ramp = np.linspace(0.0, 255.0, 32, dtype=np.float32)
    out = [np.zeros((32, 32), np.float32), np.full((32, 32), 255.0, np.float32)]
    out += [np.random.RandomState(s).uniform(0.0, 255.0, (32, 32)).astype(np.float32) for s in range(4)]
    out += [np.tile(ramp[None, :], (32, 1)), np.tile(ramp[:, None], (1, 32))]
    for y, x in ((0, 0), (31, 31), (28, 28), (29, 29)):
        p = np.zeros((32, 32), np.float32)
        p[y, x] = 255.0
        out.append(p)
    return np.stack(out)


def snn_match(dist_matrix):
    """Nearest neighbour, second nearest among the columns that are nobody's nearest neighbour, ratio test."""
    min_dist, idx = torch.min(dist_matrix, 1)
    dist_matrix[:, idx] = 100000
    min_2nd, _ = torch.min(dist_matrix, 1)
    ratio = min_dist / (min_2nd + 1e-8)
    keep = ratio <= SNN
    return min_dist, idx, min_2nd, ratio, torch.arange(0, idx.size(0))[keep].long(), idx[keep].long()


def main():
    ns = rh.import_reference()
    import pytorch_sift
    import Losses
    import ReprojectionStuff
    aff_sd, ori_sd = rh.load_state_dict("AffNet.pth"), rh.load_state_dict("OriNet.pth")
    A = ns.architectures.AffNetFast(PS=32); A.load_state_dict(aff_sd); A.eval()
    O = ns.architectures.OriNetFast(PS=32); O.load_state_dict(ori_sd); O.eval()
    sift = pytorch_sift.SIFTNet(patch_size=32)
    sift.eval()
    out, feats = {}, []
    for name in ("graf_img1.png", "graf_img6.png"):
        x = load_gray(os.path.join(HERE, name))
        det = ns.SparseImgRepresenter.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=500, border=5, num_Baum_iters=1,
                                                                      AffNet=A, OriNet=O)
        with torch.no_grad(), rh.quiet():
            L, r = det(x, do_ori=True)
            P = det.extract_patches_from_pyr(L, PS=32)
            D = sift(P)
        feats.append((L, r, P, D))
    (L1, r1, P1, D1), (L2, r2, P2, D2) = feats
    edge = edge_patches()
    with torch.no_grad():
        edge_desc = sift(torch.from_numpy(edge).unsqueeze(1))
    gk = sift.gk.detach().cpu().numpy().astype(np.float32)
    pk = sift.pk[0].weight.detach().numpy().reshape(11, 11).astype(np.float32)
    H = torch.from_numpy(np.loadtxt(os.path.join(HERE, "graf_H1to6p"))).float()
    min_dist, idx, min_2nd, ratio, tent1, tent2 = snn_match(Losses.distance_matrix_vector(D1, D2))
    gd, plain, in2 = ReprojectionStuff.get_GT_correspondence_indexes(L1[tent1], L2[tent2], H, dist_threshold=6)
    # the reference's fp32 result against the float64 restatement, over every patch of the file
    allp = np.concatenate([P1.numpy()[:, 0], P2.numpy()[:, 0], edge])
    alld = np.concatenate([D1.numpy(), D2.numpy(), edge_desc.numpy()])
    err = np.abs(sift_fp64(allp, gk, pk) - alld).max(axis=1)
    out.update(LAFs1=L1.numpy(), LAFs2=L2.numpy(), resp1=r1.numpy(), resp2=r2.numpy(), desc1=D1.numpy(), desc2=D2.numpy(), H=H.numpy(),
               patches1=P1.numpy()[:N_PATCHES, 0], patches2=P2.numpy()[:N_PATCHES, 0], edge_patches=edge, edge_desc=edge_desc.numpy(),
               gk=gk, pk=pk, min_dist=min_dist.numpy(), idx=idx.numpy(), min_2nd=min_2nd.numpy(), ratio=ratio.numpy(),
               tent1=tent1.numpy(), tent2=tent2.numpy(), gt_plain=plain.numpy(), gt_idx=in2.numpy(),
               ref_err_fp64=np.float64(err.max()))
    path = os.path.join(HERE, "sift_graf16_n500.npz")
    np.savez_compressed(path, **out)
    near = np.abs(ratio.numpy() - SNN) < NEAR
    print("tentatives %d, homography-consistent %d" % (tent1.numel(), plain.numel()))
    print("rows with |ratio - %.1f| < %.0e: %d; closest %.2e" % (SNN, NEAR, int(near.sum()), float(np.abs(ratio.numpy() - SNN).min())))
    print("reference fp32 vs float64 restatement: max %.3g, 99th percentile per row %.3g; edge cases max %.3g"
          % (err.max(), np.percentile(err, 99), err[-len(edge):].max()))
    rs = np.random.RandomState(0)
    n1 = torch.from_numpy(D1.numpy() + rs.normal(0, 1e-4, D1.shape).astype(np.float32))
    n2 = torch.from_numpy(D2.numpy() + rs.normal(0, 1e-4, D2.shape).astype(np.float32))
    _, _, _, _, t1n, t2n = snn_match(Losses.distance_matrix_vector(n1, n2))
    same = set(zip(t1n.tolist(), t2n.tolist())) == set(zip(tent1.tolist(), tent2.tolist()))
    print("Gaussian noise 1e-4 on both descriptor sets: %d tentatives, %s" % (t1n.numel(), "same pairs" if same else "PAIRS DIFFER"))
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
