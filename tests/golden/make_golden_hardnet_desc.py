"""Records tests/golden/hardnet_desc_n301.npy: the HardNet descriptors (301 x 128 float32) that the library built from the checked-out
tree returns on the MI355X for the fixed batch of tests/test_gpu_winograd_packed.py (hardnet_fixture_batch below).

The committed file was recorded with the library of the commit BEFORE the packed Winograd weights (U = G g G^T computed in the loop
from the fp32 taps); the test asks later libraries for the same bits.  To regenerate: check out the commit whose results are to be
kept, build, and on the GPU run

    python tests/golden/make_golden_hardnet_desc.py [OUT.npy]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "hardnet_desc_n301.npy")


def hardnet_fixture_batch():
    """301 patches (ragged: not a multiple of anything the kernels tile by): 298 seeded random ones and the three degenerate patches of
    tests/test_gpu_winograd.py (left half zero, top half zero, constant)."""
    g = torch.Generator().manual_seed(20260)
    p = torch.rand(298, 1, 32, 32, generator=g) * 255
    g = torch.Generator().manual_seed(7)
    half = torch.rand(1, 1, 32, 32, generator=g) * 255
    half[..., :, :16] = 0.0
    top = torch.rand(1, 1, 32, 32, generator=g) * 255
    top[..., :16, :] = 0.0
    const = torch.full((1, 1, 32, 32), 7.0)
    return torch.cat([p[:100], half, p[100:200], top, const, p[200:]])


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import affnet_amd
    assert torch.cuda.is_available(), "recording needs the MI355X"
    H = affnet_amd.HardNet(); H.load_state_dict(affnet_amd.synthetic_hardnet_state(0)); H = H.to("cuda:0")
    d = H(hardnet_fixture_batch().to("cuda:0")).cpu().numpy()
    assert d.shape == (301, 128) and d.dtype == np.float32 and np.isfinite(d).all()
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.save(out, d)
    print("wrote %s: %d x %d float32" % (out, d.shape[0], d.shape[1]))
