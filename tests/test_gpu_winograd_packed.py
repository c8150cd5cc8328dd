"""HardNet's Winograd layers read their transformed weights U = G g G^T from the packed blob and conv5 shares its window transform
through LDS (affnet_amd/csrc/cnn_mfma.h: conv3x3_wino_mfma_pair_rows, conv3x3_wino_mfma_shared_v).  Neither changes a value or the order of a sum,
so the descriptors are BIT-EQUAL to those of the library that computed U in the loop: tests/golden/hardnet_desc_n301.npy was recorded
on the MI355X from that library (tests/golden/make_golden_hardnet_desc.py says how) for the fixed batch below - 301 patches, ragged,
with the degenerate patches of tests/test_gpu_winograd.py among them."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from make_golden_hardnet_desc import hardnet_fixture_batch  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hardnet():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    H = affnet_amd.HardNet(); H.load_state_dict(affnet_amd.synthetic_hardnet_state(0))
    return H.to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
def test_descriptors_bit_equal_to_the_recorded_parent(hardnet, golden_dir):
    want = np.load(os.path.join(golden_dir, "hardnet_desc_n301.npy"))
    p = hardnet_fixture_batch()
    assert want.shape == (p.shape[0], 128) and want.dtype == np.float32
    got = hardnet(p.to(DEV)).cpu().numpy()
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print("rows that differ from the recorded descriptors: %d of %d, max |diff| = %.3g" % (bad.size, want.shape[0], d))
    assert bad.size == 0, (bad[:8], d)


@pytest.mark.gpu
def test_descriptors_bit_equal_run_to_run_and_across_batch_splits(hardnet):
    """Same bits on a second run, and a patch's descriptor does not depend on which batch it travels in (one workgroup per patch)."""
    p = hardnet_fixture_batch().to(DEV)
    a = hardnet(p)
    b = hardnet(p)
    c = torch.cat([hardnet(p[:77]), hardnet(p[77:])])
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a, c)
