"""Golden vectors for the ellipse reader, from the UNMODIFIED reference function LAF.ells2LAFsT (LAF.py:76-89, with invSqrtTorch :52-74
and rectifyAffineTransformationUpIsUp :285-291) on CPU fp32:
  * the 600 Oxford ellipses of handcrafted_slots.npz (default_ellT + baum16_ellT: what hesaffnet.py / hesaffBaum.py write);
  * three hand-made rows with b = 0 (the `mask` branch of invSqrtTorch): a circle and two axis-aligned ellipses.

    python tests/golden/make_golden_ells.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402


def main():
    ns = rh.import_reference()
    hc = np.load(os.path.join(HERE, "handcrafted_slots.npz"))
    hand = np.array([[50.0, 60.0, 0.01, 0.0, 0.01],           # circle, radius 10
                     [120.5, 33.25, 0.04, 0.0, 0.0025],       # axes 5 (x) and 20 (y)
                     [7.0, 200.0, 0.000625, 0.0, 0.0625]],    # axes 40 (x) and 4 (y)
                    dtype=np.float32)
    ells = np.concatenate([hc["default_ellT"], hc["baum16_ellT"], hand]).astype(np.float32)
    with torch.no_grad(), rh.quiet():
        lafs = ns.LAF.ells2LAFsT(torch.from_numpy(ells.copy()))
    assert lafs.dtype == torch.float32
    np.savez_compressed(os.path.join(HERE, "ells2lafs.npz"), ells=ells, lafs=lafs.numpy())
    print("written: %d ellipses (%d with b == 0)" % (len(ells), int((ells[:, 3] == 0).sum())))


if __name__ == "__main__":
    main()
