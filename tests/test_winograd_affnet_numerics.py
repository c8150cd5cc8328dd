"""CPU pins of the Winograd F(2x2, 3x3) arithmetic in the AffNet / OriNet trunks (tools/winograd_numerics.py mirrors the transform order of
affnet_amd/csrc/cnn_mfma.h: conv3x3_wino_mfma_rows): against a float64 forward, the fp32 Winograd trunk is at most twice as far as the fp32
direct trunk, per layer and at the pooled head output.  The OriNet kernel runs conv1 and conv3 as Winograd (AffNet's stays direct because of the
shape filter's sensitivity, not because of this error); conv1 / conv3 / conv5 is pinned as well (same transforms, one layer more).  Both sides of the ratio are computed here; nothing is stored."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import winograd_numerics as wn  # noqa: E402


@pytest.mark.parametrize("layers", [(1, 3), (1, 3, 5)])
@pytest.mark.parametrize("net", ["affnet", "orinet"])
def test_winograd_error_within_twice_the_direct_fp32_error(net, layers):
    sd = wn.load_net16(net)
    golden = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "cnn_random_patches.npz"))["patches"]).reshape(-1, 1, 32, 32)
    for tag, p in (("golden", golden), ("smooth", wn.smooth_patches(2000, 1))):
        e = wn.errors16(sd, p, net, layers)
        d, w = e["direct"], e["winograd"]
        print("%s %s layers %s: direct %s head %.3g | winograd %s head %.3g" % (net, tag, layers, ["%.2g" % v for v in d["layers"]], d["head"],
                                                                                ["%.2g" % v for v in w["layers"]], w["head"]))
        for li in range(6):
            if li < min(layers):
                assert w["layers"][li] == d["layers"][li]            # in front of the first Winograd layer the two trunks are the same code
            assert w["layers"][li] <= 2.0 * d["layers"][li], (tag, li, w["layers"][li], d["layers"][li])
        assert w["head"] <= 2.0 * d["head"], (tag, w["head"], d["head"])
        assert w["head"] < 2e-6                                      # an order under the 2e-5 bar of the GPU test on these outputs
