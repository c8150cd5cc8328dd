#!/usr/bin/env python
"""Describe somebody else's keypoints (MI355X): AffNet shape, OriNet orientation and a descriptor for the regions of an Oxford
ellipse file - the flow of the reference's examples/SIFT-AffNet-HardNet-kornia-matching.ipynb with this library's fused path.

    python describe_keypoints.py IMAGE ELLIPSES.txt OUT [--desc hardnet|sift] [--hardnet CHECKPOINT] [--no-shape] [--no-ori]

ELLIPSES.txt = the file hesaffnet.py writes: line 1 "1.0", line 2 the count, then one `x y a b c` row per region (the ellipse is the
whole measurement region).  Writes OUT in the same format (the regions after shape estimation, at the centres of the input file;
regions the shape filter rejects are dropped), OUT.desc.npy with the (N,128) descriptors and OUT.rows.npy with the input row of every
output row.
HardNet++.pth is not part of the reference snapshot: without --hardnet seeded synthetic weights are used."""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, REPO)
import affnet_amd  # noqa: E402
from affnet_amd.LAF import LAFs2ellT, ells2LAFs  # noqa: E402
from affnet_amd.pytorch_sift import SIFTNet  # noqa: E402


def read_gray(path):
    """RGB -> per-pixel channel mean, float32 0..255, shape (1,1,H,W) (hesaffnet.py:35-39)."""
    rgb = np.asarray(Image.open(path).convert("RGB"), dtype=np.float64)
    return torch.from_numpy(rgb.mean(axis=2).astype(np.float32))[None, None]


def read_oxford(path):
    ells = np.loadtxt(path, skiprows=2, ndmin=2)
    if ells.shape[1] != 5:
        raise ValueError("%s: expected rows of `x y a b c`" % path)
    return ells


def load(net, name):
    net.load_state_dict(torch.load(os.path.join(REPO, "pretrained", name), map_location="cpu", weights_only=False)["state_dict"])
    return net


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("image"); ap.add_argument("ellipses"); ap.add_argument("out")
    ap.add_argument("--desc", choices=("hardnet", "sift"), default="hardnet")
    ap.add_argument("--hardnet", default=None, help="HardNet checkpoint (state_dict)")
    ap.add_argument("--no-shape", action="store_true", help="keep the ellipses' shape (no AffNet, no shape filter)")
    ap.add_argument("--no-ori", action="store_true", help="keep the up-is-up orientation (no OriNet)")
    a = ap.parse_args(argv)
    ells = read_oxford(a.ellipses)
    if a.desc == "sift":
        descriptor = SIFTNet(patch_size=32)
    else:
        descriptor = affnet_amd.HardNet()
        if a.hardnet:
            descriptor.load_state_dict(torch.load(a.hardnet, map_location="cpu", weights_only=False)["state_dict"])
        else:
            print("no HardNet checkpoint given: seeded synthetic HardNet weights")
            descriptor.load_state_dict(affnet_amd.synthetic_hardnet_state(0))
    extractor = affnet_amd.ScaleSpaceAffinePatchExtractor(num_features=len(ells), num_Baum_iters=0 if a.no_shape else 1,
                                                          AffNet=load(affnet_amd.AffNetFast(PS=32), "AffNet.pth"),
                                                          OriNet=load(affnet_amd.OriNetFast(PS=32), "OriNet.pth")).cuda()
    frames = torch.from_numpy(ells2LAFs(ells).astype(np.float32)).cuda()
    with torch.no_grad():
        r = extractor.describe_frames(read_gray(a.image).cuda(), frames, do_ori=not a.no_ori, desc=descriptor.cuda())
        out = LAFs2ellT(r["LAFs"]).cpu().numpy().astype(np.float64)
    rows = r["ids"][:, 2].cpu().numpy()
    # describing a keypoint does not move it: the file carries the caller's own centres (the frames' centres went through fp32
    # normalisation by the image size and back, which is not exact to the last bit)
    out[:, :2] = ells[rows, :2]
    with open(a.out, "w") as f:
        f.write("1.0\n%d\n" % len(out))
        np.savetxt(f, out, delimiter=" ", fmt="%10.10f")
    np.save(a.out + ".desc.npy", r["descriptors"].cpu().numpy())
    np.save(a.out + ".rows.npy", rows)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
