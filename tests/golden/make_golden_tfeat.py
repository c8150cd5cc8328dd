"""Golden vectors for the HardTFeat descriptor: the UNMODIFIED reference HardTFeatNet (HardNet.py:30-59) on CPU with
the trained weights of the reference's HardTFeat.pth, loaded where they lie through oracle/ref_harness.py, and the matching steps of
train_AffNet_test_on_graffity.py:292-305 on its descriptors (make_golden_sift.snn_match on the reference's own distance matrix).

    python tests/golden/make_golden_tfeat.py   -> tests/golden/tfeat_graf16_n500.npz, tfeat_weights_{0,1,2}.npz

The geometry is the SIFT fixture's (graf img1 / img6, 500 keypoints, mrSize 5.192, border 5, shipped AffNet + OriNet, do_ori): LAFs,
responses, the first 32 patches per image and the twelve edge-case patches are asserted bit-equal to sift_graf16_n500.npz and are read
from there by the tests instead of being stored twice.  The six learned tensors go out as exact float32, split by classifier output
channel into three files.  Runs only where the reference is available; nothing of it is copied."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
from make_golden import load_gray  # noqa: E402
from make_golden_sift import N_PATCHES, NEAR, SNN, edge_patches, snn_match  # noqa: E402
from _tfeat_fp64 import KEYS, tfeat_fp64  # noqa: E402

CLS_SPLIT = (0, 32, 80, 128)          # classifier output channels per weight file (the first file also holds the features)


def main():
    ns = rh.import_reference()
    import pytorch_sift
    import Losses
    import ReprojectionStuff
    aff_sd, ori_sd = rh.load_state_dict("AffNet.pth"), rh.load_state_dict("OriNet.pth")
    A = ns.architectures.AffNetFast(PS=32); A.load_state_dict(aff_sd); A.eval()
    O = ns.architectures.OriNetFast(PS=32); O.load_state_dict(ori_sd); O.eval()
    ck = torch.load(os.path.join(rh.REF_ROOT, "HardTFeat.pth"), map_location="cpu", weights_only=False)
    net = ns.HardNet.HardTFeatNet(sm=pytorch_sift.SIFTNet(patch_size=32))
    missing = net.load_state_dict(ck["state_dict"])
    assert not missing.missing_keys and not missing.unexpected_keys, missing
    net.eval()
    sd = {k: ck["state_dict"][k].detach().cpu().numpy().astype(np.float32) for k in KEYS}
    feats = []
    for name in ("graf_img1.png", "graf_img6.png"):
        x = load_gray(os.path.join(HERE, name))
        det = ns.SparseImgRepresenter.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=500, border=5, num_Baum_iters=1,
                                                                      AffNet=A, OriNet=O)
        with torch.no_grad(), rh.quiet():
            L, r = det(x, do_ori=True)
            P = det.extract_patches_from_pyr(L, PS=32)
            D = net(P)
        feats.append((L, r, P, D))
    (L1, r1, P1, D1), (L2, r2, P2, D2) = feats
    edge = edge_patches()
    with torch.no_grad():
        edge_desc = net(torch.from_numpy(edge).unsqueeze(1))
    s = np.load(os.path.join(HERE, "sift_graf16_n500.npz"))
    for key, val in (("LAFs1", L1), ("LAFs2", L2), ("resp1", r1), ("resp2", r2)):
        assert s[key].tobytes() == val.numpy().tobytes(), key
    assert s["patches1"].tobytes() == P1.numpy()[:N_PATCHES, 0].tobytes() and s["patches2"].tobytes() == P2.numpy()[:N_PATCHES, 0].tobytes()
    assert s["edge_patches"].tobytes() == edge.tobytes()
    H = torch.from_numpy(np.loadtxt(os.path.join(HERE, "graf_H1to6p"))).float()
    assert H.numpy().tobytes() == s["H"].tobytes()
    min_dist, idx, min_2nd, ratio, tent1, tent2 = snn_match(Losses.distance_matrix_vector(D1, D2))
    gd, plain, in2 = ReprojectionStuff.get_GT_correspondence_indexes(L1[tent1], L2[tent2], H, dist_threshold=6)
    # the reference's fp32 result against the float64 referee, over every patch of the run and over the 76 patches the GPU test uses
    allp = np.concatenate([P1.numpy()[:, 0], P2.numpy()[:, 0], edge])
    alld = np.concatenate([D1.numpy(), D2.numpy(), edge_desc.numpy()])
    err = np.abs(tfeat_fp64(allp, sd) - alld).max(axis=1)
    out = dict(desc1=D1.numpy(), desc2=D2.numpy(), edge_desc=edge_desc.numpy(), H=H.numpy(), min_dist=min_dist.numpy(), idx=idx.numpy(),
               min_2nd=min_2nd.numpy(), ratio=ratio.numpy(), tent1=tent1.numpy(), tent2=tent2.numpy(), gt_plain=plain.numpy(), gt_idx=in2.numpy(),
               ref_err_fp64=np.float64(err.max()))
    path = os.path.join(HERE, "tfeat_graf16_n500.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    for i in range(3):
        lo, hi = CLS_SPLIT[i], CLS_SPLIT[i + 1]
        part = {"classifier.1.weight.part": sd[KEYS[4]][lo:hi]}
        if i == 0:
            part.update({k: sd[k] for k in KEYS[:4]})
        if i == 2:
            part[KEYS[5]] = sd[KEYS[5]]
        wpath = os.path.join(HERE, "tfeat_weights_%d.npz" % i)
        np.savez_compressed(wpath, **part)
        print("wrote %s (%d bytes)" % (wpath, os.path.getsize(wpath)))
    near = np.abs(ratio.numpy() - SNN) < NEAR
    print("tentatives %d, homography-consistent %d" % (tent1.numel(), plain.numel()))
    print("rows with |ratio - %.1f| < %.0e: %d; closest %.2e" % (SNN, NEAR, int(near.sum()), float(np.abs(ratio.numpy() - SNN).min())))
    sel = np.r_[0:N_PATCHES, 500:500 + N_PATCHES, 1000:1000 + len(edge)]
    print("reference fp32 vs float64 referee: max %.3g over %d patches, 99th percentile per row %.3g; the 76 test patches %.3g"
          % (err.max(), len(err), np.percentile(err, 99), err[sel].max()))
    rs = np.random.RandomState(0)
    n1 = torch.from_numpy(D1.numpy() + rs.normal(0, 1e-4, D1.shape).astype(np.float32))
    n2 = torch.from_numpy(D2.numpy() + rs.normal(0, 1e-4, D2.shape).astype(np.float32))
    _, _, _, _, t1n, t2n = snn_match(Losses.distance_matrix_vector(n1, n2))
    same = set(zip(t1n.tolist(), t2n.tolist())) == set(zip(tent1.tolist(), tent2.tolist()))
    print("Gaussian noise 1e-4 on both descriptor sets: %d tentatives, %s" % (t1n.numel(), "same pairs" if same else "PAIRS DIFFER"))


if __name__ == "__main__":
    main()
