"""CPU pin of the arithmetic of the exact OriNet trunk with conv1, conv3 AND conv5 as Winograd F(2x2, 3x3) (tools/winograd_numerics.py mirrors the transform
order of affnet_amd/csrc/cnn_mfma.h; conv5's wave pairs combine their position rows in wino_output's order, so wino_conv3x3 is its mirror as well): against a
float64 forward, every layer and the pooled head of the fp32 Winograd trunk are at most twice as far as the fp32 direct trunk on the same input - the bar of
tests/test_winograd_affnet_numerics.py.  Both sides of the ratio are computed here; nothing is stored."""
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

BAR = 2.0        # tests/test_winograd_affnet_numerics.py


@pytest.mark.parametrize("tag", ["golden", "smooth"])
def test_orinet_conv1_conv3_conv5_within_twice_the_direct_fp32_error(tag):
    assert wn.WINO_LAYERS_16 == (1, 3, 5)
    sd = wn.load_net16("orinet")
    if tag == "golden":
        p = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "cnn_random_patches.npz"))["patches"]).reshape(-1, 1, 32, 32)
    else:
        p = wn.smooth_patches(1000, 1)
    e = wn.errors16(sd, p, "orinet")                             # the tool's default layers: what the kernel runs
    d, w = e["direct"], e["winograd"]
    print("orinet %s: direct %s head %.3g angle %.3g | winograd %s head %.3g angle %.3g" % (
        tag, ["%.2g" % v for v in d["layers"]], d["head"], d["angle"], ["%.2g" % v for v in w["layers"]], w["head"], w["angle"]))
    assert w["layers"][0] == d["layers"][0]                      # conv0 is the same code in both trunks
    for li in range(6):
        assert w["layers"][li] <= BAR * d["layers"][li], (tag, li, w["layers"][li], d["layers"][li])
    assert w["head"] <= BAR * d["head"], (tag, w["head"], d["head"])
