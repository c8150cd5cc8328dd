"""CPU checks of the HardTFeat descriptor's host side: the float64 referee against the unmodified reference's
golden descriptors, the weight packer through the documented index functions of csrc/weights_layout.h, the mirror class's state-dict
contract and refusals, and the conditions the golden fixture has to meet so that the GPU matching test (tests/test_gpu_tfeat.py) cannot
hide a failure."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _tfeat_fp64 import KEYS, load_golden_weights, random_state_dict, tfeat_fp64


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "tfeat_graf16_n500.npz"))


@pytest.fixture(scope="module")
def sift_g(golden_dir):
    return np.load(os.path.join(golden_dir, "sift_graf16_n500.npz"))          # the geometry and the patches are the SIFT fixture's


@pytest.fixture(scope="module")
def trained(golden_dir):
    return load_golden_weights(golden_dir)


@pytest.fixture(scope="module")
def patches(sift_g):
    return np.concatenate([sift_g["patches1"], sift_g["patches2"], sift_g["edge_patches"]]).astype(np.float32)


def test_referee_agrees_with_every_golden_descriptor(g, trained, patches):
    want = np.concatenate([g["desc1"][:32], g["desc2"][:32], g["edge_desc"]])
    got = tfeat_fp64(patches, trained)
    err = float(np.abs(got - want).max())
    print("referee vs golden: %.3g (the reference's own distance, ref_err_fp64 = %.3g)" % (err, float(g["ref_err_fp64"])))
    assert err <= 2.0 * float(g["ref_err_fp64"])
    assert float(g["ref_err_fp64"]) <= 5e-7                                    # fp32 chains of 49 / 1152 / 4096 terms against float64
    # a flat patch is exactly zero after the input norm (0 / 1e-7): finite, and the same for all-0 and all-255
    assert np.isfinite(g["edge_desc"]).all() and np.array_equal(g["edge_desc"][0], g["edge_desc"][1])
    assert np.array_equal(got[64], got[65])
    assert np.abs(np.sqrt((got ** 2).sum(1)) - 1.0).max() < 1e-6


def _unpack(blob):
    """The six tensors from the packed blob, by the index functions of csrc/weights_layout.h: conv1 [k = ky * 7 + kx (52)][n] (tfeat_c1_index),
    conv2 [tap p = ky * 6 + kx][c / 16][(c / 4) % 4][n][c % 4] (tfeat_c2_index = w_tap_index), classifier [k / 16][(k / 4) % 4][n][k % 4] with
    k = pixel * 64 + c (tfeat_head_index), each followed by its bias."""
    off = 0
    c1 = blob[off:off + 52 * 32].reshape(52, 32); off += 52 * 32
    b1 = blob[off:off + 32]; off += 32
    c2 = blob[off:off + 36 * 32 * 64].reshape(36, 2, 4, 64, 4); off += 36 * 32 * 64
    b2 = blob[off:off + 64]; off += 64
    hw = blob[off:off + 4096 * 128].reshape(256, 4, 128, 4); off += 4096 * 128
    hb = blob[off:off + 128]; off += 128
    assert off == blob.size
    assert not c1[49:].any()                                                   # the K padding: zero weights
    w1 = c1[:49].T.reshape(32, 1, 7, 7)
    w2 = c2.transpose(3, 1, 2, 4, 0).reshape(64, 32, 6, 6)                     # [n][G][kq][j][p] -> c = 16 G + 4 kq + j
    wh = hw.transpose(2, 0, 1, 3).reshape(128, 64, 64).transpose(0, 2, 1).reshape(128, 64, 8, 8)      # [n][k] -> [n][pixel][c] -> [n][c][y][x]
    return dict(zip(KEYS, (w1, b1, w2, b2, wh, hb)))


def _pack(sd):
    from affnet_amd import _lib
    n = _lib.lib.affnet_tfeat_packed_floats()
    assert n == 52 * 32 + 32 + 36 * 32 * 64 + 64 + 4096 * 128 + 128
    blob = np.full(n, np.nan, np.float32)                                      # every float must be written
    t = [np.ascontiguousarray(sd[k], dtype=np.float32) for k in KEYS]
    rc = _lib.lib.affnet_tfeat_pack_weights(*([x.ctypes.data_as(C.c_void_p) for x in t] + [blob.ctypes.data_as(C.c_void_p)]))
    assert rc == _lib.OK
    return blob


@pytest.mark.parametrize("which", ["trained", "random"])
def test_packed_blob_reproduces_the_network(which, trained, patches):
    sd = trained if which == "trained" else random_state_dict(0)
    blob = _pack(sd)
    assert np.isfinite(blob).all()
    un = _unpack(blob)
    for k in KEYS:
        assert un[k].shape == sd[k].shape and np.array_equal(un[k], sd[k]), k    # every weight exactly where the documented order says
    want, got = tfeat_fp64(patches, sd), tfeat_fp64(patches, un)
    assert float(np.abs(got - want).max()) <= 1e-12
    if which == "random":
        # the seeded weights keep the tanh layers out of saturation and move every asymmetric patch: a transposed filter cannot hide
        t = dict(sd)
        t[KEYS[2]] = np.ascontiguousarray(sd[KEYS[2]].transpose(0, 1, 3, 2))
        assert float(np.abs(tfeat_fp64(patches[:64], t) - want[:64]).max(axis=1).min()) > 1e-3


def test_pack_refuses_null_arguments():
    from affnet_amd import _lib
    buf = (C.c_float * 4)()
    assert _lib.lib.affnet_tfeat_pack_weights(None, buf, buf, buf, buf, buf, buf) == _lib.ERR_INVALID
    assert _lib.lib.affnet_tfeat_pack_weights(buf, buf, buf, buf, buf, buf, None) == _lib.ERR_INVALID
    assert _lib.lib.affnet_tfeat_scratch_floats(0) == 0 and _lib.lib.affnet_tfeat_scratch_floats(-3) == 0
    assert _lib.lib.affnet_tfeat_scratch_floats(10) == 10 * (4096 + 4 * 128)
    assert _lib.lib.affnet_tfeat_forward(None, buf, buf, None, 1, buf, buf, None) == _lib.ERR_INVALID
    assert _lib.lib.affnet_tfeat_forward_pyr(None, buf, buf, buf, None, 1, buf, buf, None) == _lib.ERR_INVALID


def test_mirror_loads_the_reference_state_dict(trained):
    import affnet_amd
    from affnet_amd.HardNet import HardTFeatNet
    assert affnet_amd.HardTFeatNet is HardTFeatNet
    sift = affnet_amd.SIFTNet(patch_size=32)
    net = affnet_amd.HardTFeatNet(sm=sift)
    assert net.PS == 32 and net.SIFT is sift and not net.training
    ck = {k: torch.from_numpy(v) for k, v in trained.items()}
    # the reference checkpoint also holds the SIFT module's three fixed filters, which forward() never uses
    ck.update({"SIFT.gx.0.weight": torch.zeros(1, 1, 1, 3), "SIFT.gy.0.weight": torch.zeros(1, 1, 3, 1), "SIFT.pk.0.weight": torch.zeros(1, 1, 11, 11)})
    res = net.load_state_dict(ck)
    assert not res.missing_keys and not res.unexpected_keys
    sd = net.state_dict()
    assert tuple(sd.keys()) == KEYS
    for k in KEYS:
        assert sd[k].dtype == torch.float32 and sd[k].numpy().tobytes() == trained[k].tobytes(), k
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in ck.items() if k != KEYS[0]})      # a learned tensor missing: strict like the reference
    # the blob is cached per device and repacked when a parameter changes
    a = net.packed_weights(torch.device("cpu"))
    assert net.packed_weights(torch.device("cpu")) is a and np.array_equal(a.numpy(), _pack(trained))
    with torch.no_grad():
        net.classifier[1].bias.add_(1.0)
    b = net.packed_weights(torch.device("cpu"))
    assert b is not a and float((b[-128:] - a[-128:]).abs().min()) > 0.5


def test_refusals():
    import affnet_amd
    net = affnet_amd.HardTFeatNet(sm=None)
    with pytest.raises(RuntimeError, match="MI355X"):
        net(torch.zeros(2, 1, 32, 32))                                          # a CPU tensor: there is no CPU path
    net.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        net(torch.zeros(2, 1, 32, 32))
    net.eval()
    for mode in ("fp32_split3", "fp32_split2h"):
        net.arith = mode
        with pytest.raises(NotImplementedError, match="exact fp32"):
            net(torch.zeros(2, 1, 32, 32))
    net.arith = "fp32"
    for shape in ((2, 2, 32, 32), (2, 1, 31, 32), (2, 32, 33), (32, 32), (2, 1, 1, 32, 32)):     # the shape is checked before the device
        with pytest.raises(ValueError):
            net(torch.zeros(*shape))
    one = affnet_amd.OnePassSIR(num_features=10, AffNet=affnet_amd.AffNetFastFullConv())
    with pytest.raises(NotImplementedError, match="HardNet only"):                  # its fused call would read the blob as a HardNet blob
        one.enqueue(torch.zeros(1, 1, 64, 64), do_ori=False, desc=net)
    with pytest.raises(NotImplementedError, match="HardNet only"):
        one.enqueue(torch.zeros(1, 1, 64, 64), do_ori=False, desc=affnet_amd.SIFTNet(patch_size=32))
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(num_features=10)
    with pytest.raises(NotImplementedError, match="HardTFeat"):
        det.capture(torch.zeros(1, 1, 64, 64), desc=net)


def test_fixture_cannot_hide_a_matching_failure(g, sift_g):
    """The GPU matching test excuses tentatives whose golden ratio is within 5e-3 of the 0.8 threshold: they must be few, the counts are the
    ones the generator printed, and the geometry is the SIFT fixture's."""
    ratio = g["ratio"]
    assert np.array_equal(np.nonzero(ratio <= 0.8)[0], g["tent1"]) and np.array_equal(g["idx"][g["tent1"]], g["tent2"])
    near = int((np.abs(ratio - 0.8) < 5e-3).sum())
    print("tentatives %d, homography-consistent %d, borderline rows %d" % (len(g["tent1"]), len(g["gt_plain"]), near))
    assert (len(g["tent1"]), len(g["gt_plain"]), near) == (34, 5, 3)
    assert g["desc1"].shape == (500, 128) and g["desc2"].shape == (500, 128) and g["edge_desc"].shape == (12, 128)
    assert sift_g["resp1"].shape == (500,) and sift_g["LAFs2"].shape == (500, 2, 3) and np.array_equal(g["H"], sift_g["H"])
