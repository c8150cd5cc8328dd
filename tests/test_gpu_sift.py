"""The native SIFT descriptor (csrc/sift.hip, affnet_amd.pytorch_sift.SIFTNet) on the MI355X: the kernel against the float64
referee (tests/_sift_fp64.py) on the reference's golden patches, determinism, the pyramid form against the patches form, batches,
and graf 1-6 matching end to end against the unmodified reference's golden rows (tests/golden/sift_graf16_n500.npz)."""
import os

import numpy as np
import pytest
import torch

from _rowmatch import match_rows
from _sift_fp64 import sift_fp64
from conftest import load_gray, record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# Kernel vs referee: 8 x the reference's own distance from the referee (ref_err_fp64, 1.92e-7 -> 1.5e-6).  Device atan2f / sqrtf are a
# few ulp from the host's libm and the 121- and 128-term sums run in another order; entries are <= 0.33, and one pixel in a wrong
# bin or under a wrong border rule moves an entry by >= 1e-4: the bar separates right from wrong by two orders of magnitude.
MARGIN = 8.0
DESC_BAR = 1e-3         # the project's bar for full-path descriptors (tests/test_gpu_parity.py)
NEAR = 5e-3             # |golden ratio - 0.8| below which a tentative may flip


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "sift_graf16_n500.npz"))


@pytest.fixture(scope="module")
def cases(g):
    """The 64 + 12 golden patches and their float64 referee descriptors (computed once)."""
    patches = np.concatenate([g["patches1"], g["patches2"], g["edge_patches"]]).astype(np.float32)
    return patches, sift_fp64(patches, g["gk"], g["pk"]), sift_fp64(patches, g["gk"], g["pk"], clipval=1.0)


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    return affnet_amd


@pytest.fixture(scope="module")
def det_nets(amd, weights):
    A = amd.AffNetFast(PS=32); A.load_state_dict(weights["AffNet"])
    O = amd.OriNetFast(PS=32); O.load_state_dict(weights["OriNet"])
    return A.to(DEV), O.to(DEV)


def _extractor(amd, det_nets, n):
    return amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=n, border=5, num_Baum_iters=1, AffNet=det_nets[0], OriNet=det_nets[1]).to(DEV)


@pytest.mark.parametrize("n", [76, 1, 3, 65])
def test_kernel_against_the_referee(amd, g, cases, n):
    patches, want, _ = cases
    bar = MARGIN * float(g["ref_err_fp64"])
    net = amd.SIFTNet(patch_size=32)
    x = torch.from_numpy(patches[:n]).to(DEV)
    got = net(x.unsqueeze(1)).cpu().numpy()
    assert got.shape == (n, 128) and np.isfinite(got).all()
    err = float(np.abs(got - want[:n]).max())
    print("SIFT kernel vs float64 referee, n = %d: max abs %.3g (bar %.3g)" % (n, err, bar))
    record_parity("SIFT kernel vs float64 referee, %d golden patches" % n, max_abs=err, bar=bar, reference_vs_referee=float(g["ref_err_fp64"]))
    assert err <= bar
    assert torch.equal(net(x), net(x.unsqueeze(1)))                               # (n,32,32) and (n,1,32,32) are the same call
    if n == 76:
        # against the reference's own fp32 descriptors: its distance from the referee + ours
        ref = np.concatenate([g["desc1"][:32], g["desc2"][:32], g["edge_desc"]])
        assert float(np.abs(got - ref).max()) <= bar + float(g["ref_err_fp64"])
        # the single bright pixels at (0,0), (31,31), (28,28), (29,29) lie where the window is zero or in the unused 29..31 margin:
        # like the reference, exactly the flat patch's descriptor
        flat = got[64]
        for k in (65, 72, 73, 74, 75):
            assert np.array_equal(got[k], flat), k
        assert net(x[:0]).shape == (0, 128)


def test_margin_rows_reach_no_cell(amd, g):
    """Rows and columns 29..31 feed no cell although the window is not zero there: a bright pixel at (30,16) or (16,30) has all its
    gradients in the margin and gives the flat descriptor bit for bit; at (29,16) its vertical gradient at (28,16) reaches cells
    (3,1) and (3,2) and must agree with the referee."""
    p = np.zeros((4, 32, 32), np.float32)
    p[1, 30, 16] = p[2, 16, 30] = p[3, 29, 16] = 255.0
    got = amd.SIFTNet(patch_size=32)(torch.from_numpy(p).to(DEV)).cpu().numpy()
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[2], got[0])
    want = sift_fp64(p, g["gk"], g["pk"])
    assert np.abs(want[3] - want[0]).max() > 1e-2
    assert float(np.abs(got - want).max()) <= MARGIN * float(g["ref_err_fp64"])


def test_deterministic_and_clipval(amd, g, cases):
    patches, _, want1 = cases
    x = torch.from_numpy(patches).to(DEV)
    net, net1 = amd.SIFTNet(patch_size=32), amd.SIFTNet(patch_size=32, clipval=1.0)
    a, b = net(x), net(x)
    assert torch.equal(a, b)
    c = net1(x)
    k = 70                                                                         # the horizontal ramp: all gradient in one bin, entries
    assert float((a[k] - c[k]).abs().max()) > 5e-2                                 # up to 0.35 unclipped (the referee: 0.0896 apart)
    assert float(a[k].max()) < float(c[k].max())
    nrm = c.double().pow(2).sum(1).sqrt().cpu().numpy()
    assert np.abs(nrm - 1.0).max() < 1e-6
    assert float(np.abs(c.cpu().numpy() - want1).max()) <= MARGIN * float(g["ref_err_fp64"])      # the same bar with clipval = 1


def test_pyramid_form_equals_patches_form(amd, det_nets):
    x = amd.synthetic_image(240, 320, 1).to(DEV)
    det = _extractor(amd, det_nets, 300)
    net = amd.SIFTNet(patch_size=32)
    r = det.run(x, do_ori=True, desc=net)
    assert r["descriptors"].shape == (r["LAFs"].shape[0], 128) and r["LAFs"].shape[0] > 250
    staged = net(det.extract_patches_from_pyr(r["LAFs"], PS=32))
    assert torch.equal(r["descriptors"], staged)
    L2, D2 = amd.get_geometry_and_descriptors(x, det, net, do_ori=True)            # takes the same native path
    assert torch.equal(L2, r["LAFs"]) and torch.equal(D2, r["descriptors"])
    plain = det.run(x, do_ori=True)                                                # the geometry does not depend on the descriptor slot
    assert torch.equal(plain["LAFs"], r["LAFs"]) and plain["descriptors"] is None
    with pytest.raises(NotImplementedError):
        det.capture(x, do_ori=True, desc=net)


def test_batch_equals_single_images(amd, det_nets):
    imgs = [amd.synthetic_image(240, 320, 1), torch.full((1, 1, 240, 320), 97.0), amd.synthetic_image(240, 320, 2)]
    det = _extractor(amd, det_nets, 300)
    net = amd.SIFTNet(patch_size=32)
    out = det.run_batch(torch.cat(imgs, 0).to(DEV), do_ori=True, desc=net)
    assert len(out) == 3
    assert out[1]["LAFs"].shape[0] == 0 and tuple(out[1]["descriptors"].shape) == (0, 128)      # the constant image: no detections
    enq = det.enqueue(torch.cat(imgs, 0).to(DEV), do_ori=True, desc=net)
    assert tuple(enq["descriptors"].shape) == (3, 300, 128)
    cnt = enq["count"].cpu().tolist()
    assert not enq["descriptors"][1].any() and not enq["descriptors"][0, cnt[0]:].any()         # rows past the count are zero
    for b in (0, 2):
        one = det.run(imgs[b].to(DEV), do_ori=True, desc=net)
        assert torch.equal(one["LAFs"], out[b]["LAFs"])
        assert torch.equal(one["descriptors"], out[b]["descriptors"])


def test_graf_1_6_matching_end_to_end(amd, det_nets, g, golden_dir):
    from affnet_amd import ReprojectionStuff as RS
    det = _extractor(amd, det_nets, 500)
    net = amd.SIFTNet(patch_size=32)
    res, maps, unmatched = [], [], 0
    for k, name in ((1, "graf_img1.png"), (2, "graf_img6.png")):
        r = det.run(load_gray(os.path.join(golden_dir, name)).to(DEV), do_ori=True, desc=net)
        gi, wi = match_rows(r["responses"].cpu().numpy(), r["LAFs"].cpu().numpy(), g["resp%d" % k], g["LAFs%d" % k])
        err = float(np.abs(r["descriptors"].cpu().numpy()[gi] - g["desc%d" % k][wi]).max())
        n_rows = int(r["LAFs"].shape[0])
        print("graf image %d: %d rows, %d matched to golden rows, descriptor max abs diff %.3g" % (k, n_rows, len(gi), err))
        record_parity("SIFT full path graf img%d vs the reference's golden rows, 500 kp" % (1 if k == 1 else 6), rows=n_rows, matched=int(len(gi)),
                      desc_max_abs=err)
        assert len(gi) >= 0.99 * 500
        assert err <= DESC_BAR
        unmatched += (n_rows - len(gi)) + (500 - len(gi))
        maps.append(dict(zip(gi.tolist(), wi.tolist())))
        res.append(r)
    t1, t2, _, _ = RS.match_snn(res[0]["descriptors"], res[1]["descriptors"], 0.8)
    H = torch.from_numpy(g["H"])
    _, plain, _ = RS.get_GT_correspondence_indexes(res[0]["LAFs"][t1], res[1]["LAFs"][t2], H, dist_threshold=6)
    print("tentatives %d (reference %d), homography-consistent %d (reference %d)" % (t1.numel(), len(g["tent1"]), plain.numel(), len(g["gt_plain"])))
    record_parity("SIFT SNN matching graf 1-6 end to end, 500 kp", tentatives=int(t1.numel()), reference_tentatives=int(len(g["tent1"])),
                  consistent=int(plain.numel()), reference_consistent=int(len(g["gt_plain"])), rows_without_golden_partner=int(unmatched))
    near = np.abs(g["ratio"] - 0.8) < NEAR
    ref = set(zip(g["tent1"].tolist(), g["tent2"].tolist()))
    got, excused = set(), 0
    for a, b in zip(t1.tolist(), t2.tolist()):
        if a in maps[0] and b in maps[1]:
            got.add((maps[0][a], maps[1][b]))
        else:
            excused += 1                                   # a row without a golden partner
    have1, have2 = set(maps[0].values()), set(maps[1].values())
    bad = []
    for a, b in got ^ ref:
        if near[a] or a not in have1 or b not in have2:
            excused += 1
        else:
            bad.append((a, b, float(g["ratio"][a])))
    assert not bad, "tentatives differ from the reference's away from the threshold: %s" % bad
    allowed = int(near.sum()) + unmatched
    assert excused <= allowed and abs(int(t1.numel()) - len(ref)) <= allowed
