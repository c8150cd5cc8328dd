"""CPU checks of the SIFT descriptor's host side: the float64 referee against the reference's golden
descriptors, the host tables against the reference's, the module's constructor contract, and the conditions the golden fixture has
to meet so that the GPU matching test (tests/test_gpu_sift.py) cannot hide a failure."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _sift_fp64 import sift_fp64

# the referee's distance from the reference's fp32 result, measured when the fixture was written: 1.92e-7 on the 2 x 500 graf
# patches + 12 edge cases (make_golden_sift.py prints it); the fixture is deterministic, so this bar is derived, not tuned
REFEREE_BAR = 5e-7


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "sift_graf16_n500.npz"))


def test_referee_agrees_with_every_golden_descriptor(g):
    for patches, want in ((g["patches1"], g["desc1"][:32]), (g["patches2"], g["desc2"][:32]), (g["edge_patches"], g["edge_desc"])):
        err = np.abs(sift_fp64(patches, g["gk"], g["pk"]) - want).max()
        print("referee vs golden: %.3g" % err)
        assert err <= REFEREE_BAR
    # a flat patch is well defined: every pixel in bin 0 with weight 1e-5 gk, norm 1.  The four single bright pixels sit in the
    # corners, where the circular window is zero (row 0 and column 0 of gk are zero altogether, so the replicate border never
    # shows; (29,29) and (31,31) have no gradient inside rows / columns 0..28 either): the reference gives the flat descriptor
    flat = g["edge_desc"][0]
    assert abs(float(np.sqrt((flat.astype(np.float64) ** 2).sum())) - 1.0) < 1e-6 and np.all(flat[16:] == 0) and np.all(flat[:16] > 0)
    assert not g["gk"][0].any() and not g["gk"][:, 0].any() and g["gk"][29, 16] > 0
    for k in (1, 8, 9, 10, 11):
        assert np.array_equal(g["edge_desc"][k], flat), k


def test_host_tables_equal_the_reference_bit_for_bit(g):
    from affnet_amd import _lib, pytorch_sift
    buf = (C.c_float * 1024)()
    assert _lib.lib.affnet_sift_host_window(32, buf) == _lib.OK
    win = np.array(buf, dtype=np.float32).reshape(32, 32)
    assert win.tobytes() == g["gk"].tobytes()
    assert _lib.lib.affnet_sift_host_window(65, buf) == _lib.ERR_INVALID and _lib.lib.affnet_sift_host_window(32, None) == _lib.ERR_INVALID
    net = pytorch_sift.SIFTNet(patch_size=32)
    assert net.gk.dtype == torch.float32 and tuple(net.gk.shape) == (32, 32) and net.gk.numpy().tobytes() == g["gk"].tobytes()
    pk = pytorch_sift.getPoolingKernel(kernel_size=11)
    assert pk.shape == (11, 11) and pk.astype(np.float32).tobytes() == g["pk"].tobytes()
    assert pytorch_sift.get_bin_weight_kernel_size_and_stride(32, 4) == (11, 6)
    assert (net.bin_weight_kernel_size, net.bin_weight_stride) == (11, 6)
    assert (net.num_ang_bins, net.num_spatial_bins, net.clipval) == (8, 4, 0.2)


def test_l2norm_helper():
    from affnet_amd.pytorch_sift import L2Norm
    x = torch.tensor([[3.0, 4.0], [0.0, 0.0]])
    y = L2Norm()(x)
    assert torch.allclose(y[0], torch.tensor([0.6, 0.8])) and torch.equal(y[1], torch.zeros(2))


def test_constructor_and_input_errors():
    import affnet_amd
    assert affnet_amd.SIFTNet is affnet_amd.pytorch_sift.SIFTNet
    with pytest.raises(NotImplementedError, match="patch_size=32"):
        affnet_amd.SIFTNet()                                                # the reference's default patch_size = 65
    with pytest.raises(NotImplementedError):
        affnet_amd.SIFTNet(patch_size=32, num_ang_bins=9)
    with pytest.raises(NotImplementedError):
        affnet_amd.SIFTNet(patch_size=32, num_spatial_bins=5)
    net = affnet_amd.SIFTNet(patch_size=32)
    with pytest.raises(RuntimeError, match="MI355X"):
        net(torch.zeros(2, 1, 32, 32))                                      # a CPU tensor: there is no CPU path


def test_fixture_cannot_hide_a_matching_failure(g):
    """The GPU matching test excuses tentatives whose golden ratio is within 5e-3 of the 0.8 threshold: they must be few, and the
    golden descriptors must be as close to the referee as stated."""
    ratio = g["ratio"]
    assert np.array_equal(np.nonzero(ratio <= 0.8)[0], g["tent1"]) and np.array_equal(g["idx"][g["tent1"]], g["tent2"])
    near = int((np.abs(ratio - 0.8) < 5e-3).sum())
    print("tentatives %d, homography-consistent %d, borderline rows %d" % (len(g["tent1"]), len(g["gt_plain"]), near))
    assert near <= 0.05 * len(g["tent1"])
    assert float(g["ref_err_fp64"]) <= REFEREE_BAR
    assert g["desc1"].shape == (500, 128) and g["desc2"].shape == (500, 128) and g["resp1"].shape == (500,) and g["LAFs2"].shape == (500, 2, 3)
