"""CPU pins of the Winograd F(2x2, 3x3) arithmetic of HardNet's conv1 / conv3 / conv5 (tools/winograd_numerics.py mirrors the kernel's
transform order): the algebra equals direct convolution in float64, and in fp32 it adds no more error to the descriptors than direct
fp32 convolution does."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402
import winograd_numerics as wn  # noqa: E402


def test_winograd_algebra_equals_direct_convolution_in_fp64():
    g = torch.Generator().manual_seed(3)
    for cin, cout, h in ((32, 32, 32), (64, 64, 16), (128, 128, 8)):
        x = torch.randn(2, cin, h, h, generator=g, dtype=torch.float64)
        w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
        want = F.conv2d(x, w, None, padding=1)
        assert float((wn.wino_conv3x3(x, w) - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))


def test_winograd_descriptor_error_matches_direct_fp32():
    sd = orc.synthetic_hardnet_state(0)
    golden = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "cnn_random_patches.npz"))["patches"])
    rand = torch.rand(2000, 1, 32, 32, generator=torch.Generator().manual_seed(0)) * 255
    e = wn.errors(sd, torch.cat([rand, golden.reshape(-1, 1, 32, 32)]))
    print("max |desc - fp64|: direct fp32 %.3g, Winograd fp32 %.3g" % (e["direct"][0], e["winograd"][0]))
    assert e["winograd"][0] <= 1.5 * e["direct"][0]
    assert e["winograd"][0] < 1e-6
