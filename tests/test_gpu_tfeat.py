"""The native HardTFeat descriptor (csrc/tfeat.hip, affnet_amd.HardTFeatNet) on the MI355X: the kernels against the float64 referee
(tests/_tfeat_fp64.py) on the reference's golden patches with the trained and with seeded random weights, determinism, the pyramid form
against the patches form, batches, caller-supplied frames, the arithmetic modes, and graf 1-6 matching end to end against the unmodified
reference's golden rows (tests/golden/tfeat_graf16_n500.npz; geometry and patches: sift_graf16_n500.npz)."""
import os

import numpy as np
import pytest
import torch

from _rowmatch import match_rows
from _tfeat_fp64 import load_golden_weights, random_state_dict, tfeat_fp64
from conftest import load_gray, record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# Kernel vs referee: 8 x the reference's own distance from the referee (ref_err_fp64, 2.84e-7 -> 2.27e-6), the SIFT test's convention: fp32
# chains of 49 / 1152 / 4 x 1024 terms in another order than the reference's, and a device tanhf a few ulp from the host's.  A transposed
# conv2 filter moves every graf patch by > 1e-3 with the random weights (tests/test_tfeat_host.py): three orders of magnitude above the
# bar.  Measured on an MI355X: 4.15e-7 with the trained weights, 3.89e-7 with the random ones.
MARGIN = 8.0
DESC_BAR = 1e-3         # the project's bar for full-path descriptors (tests/test_gpu_parity.py)
NEAR = 5e-3             # |golden ratio - 0.8| below which a tentative may flip


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "tfeat_graf16_n500.npz"))


@pytest.fixture(scope="module")
def sg(golden_dir):
    return np.load(os.path.join(golden_dir, "sift_graf16_n500.npz"))


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    return affnet_amd


@pytest.fixture(scope="module")
def state(golden_dir):
    return {"trained": load_golden_weights(golden_dir), "random": random_state_dict(0)}


@pytest.fixture(scope="module")
def cases(sg, state):
    """The 64 + 12 golden patches and their float64 referee descriptors per weight set (computed once)."""
    patches = np.concatenate([sg["patches1"], sg["patches2"], sg["edge_patches"]]).astype(np.float32)
    return patches, {k: tfeat_fp64(patches, sd) for k, sd in state.items()}


def _net(amd, sd):
    net = amd.HardTFeatNet(sm=amd.SIFTNet(patch_size=32))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV)


@pytest.fixture(scope="module")
def net(amd, state):
    return _net(amd, state["trained"])


@pytest.fixture(scope="module")
def det_nets(amd, weights):
    A = amd.AffNetFast(PS=32); A.load_state_dict(weights["AffNet"])
    O = amd.OriNetFast(PS=32); O.load_state_dict(weights["OriNet"])
    return A.to(DEV), O.to(DEV)


def _extractor(amd, det_nets, n, **kw):
    return amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=n, border=5, num_Baum_iters=1, AffNet=det_nets[0], OriNet=det_nets[1], **kw).to(DEV)


@pytest.mark.parametrize("which", ["trained", "random"])
@pytest.mark.parametrize("n", [76, 1, 3, 65])
def test_kernel_against_the_referee(amd, g, state, cases, n, which):
    """n = 76: two head tiles, the second with 12 rows; 1 and 3: a partial tile; 65: one row past the head's 64-patch edge.  Every patch
    runs conv1's 43 pixel tiles, the last with one valid pool window."""
    patches, want = cases[0], cases[1][which]
    bar = MARGIN * float(g["ref_err_fp64"])
    net = _net(amd, state[which])
    x = torch.from_numpy(patches[:n]).to(DEV)
    got = net(x.unsqueeze(1)).cpu().numpy()
    assert got.shape == (n, 128) and np.isfinite(got).all()
    err = float(np.abs(got - want[:n]).max())
    print("HardTFeat kernel vs float64 referee, %s weights, n = %d: max abs %.3g (bar %.3g)" % (which, n, err, bar))
    record_parity("HardTFeat kernel vs float64 referee, %s weights, %d golden patches" % (which, n), max_abs=err, bar=bar,
                  reference_vs_referee=float(g["ref_err_fp64"]))
    assert err <= bar
    assert torch.equal(net(x), net(x.unsqueeze(1)))                               # (n,32,32) and (n,1,32,32) are the same call
    if n == 76:
        assert np.array_equal(got[64], got[65])                                    # all 0 and all 255: exactly zero after the input norm
        assert abs(float(np.sqrt((got[64].astype(np.float64) ** 2).sum())) - 1.0) < 1e-6
        assert net(x[:0]).shape == (0, 128) and net(x[:0].unsqueeze(1)).shape == (0, 128)
        if which == "trained":
            # against the reference's own fp32 descriptors: its distance from the referee + ours
            ref = np.concatenate([g["desc1"][:32], g["desc2"][:32], g["edge_desc"]])
            assert float(np.abs(got - ref).max()) <= bar + float(g["ref_err_fp64"])


def test_deterministic_and_independent_of_the_batch(net, cases):
    x = torch.from_numpy(cases[0]).to(DEV)
    a, b = net(x), net(x)
    assert torch.equal(a, b)
    rows = torch.cat([net(x[k:k + 1]) for k in range(x.size(0))], 0)               # each patch alone: row 0 of its own tile
    assert torch.equal(a, rows)
    assert torch.equal(net(x.flip(0)).flip(0), a)                                  # another position in the tile, another tile
    old = net.CHUNK
    try:
        net.CHUNK = 40                                                             # two launches instead of one
        assert torch.equal(net(x), a)
    finally:
        net.CHUNK = old


def test_pyramid_form_equals_patches_form(amd, det_nets, net):
    x = amd.synthetic_image(240, 320, 1).to(DEV)
    det = _extractor(amd, det_nets, 300)
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


def test_batch_equals_single_images(amd, det_nets, net):
    imgs = [amd.synthetic_image(240, 320, 1), torch.full((1, 1, 240, 320), 97.0), amd.synthetic_image(240, 320, 2)]
    det = _extractor(amd, det_nets, 300)
    out = det.run_batch(torch.cat(imgs, 0).to(DEV), do_ori=True, desc=net)
    assert len(out) == 3
    assert out[1]["LAFs"].shape[0] == 0 and tuple(out[1]["descriptors"].shape) == (0, 128)      # the constant image: no detections
    enq = det.enqueue(torch.cat(imgs, 0).to(DEV), do_ori=True, desc=net)
    assert tuple(enq["descriptors"].shape) == (3, 300, 128)
    cnt = enq["count"].cpu().tolist()
    assert not enq["descriptors"][1].any() and not enq["descriptors"][0, cnt[0]:].any()         # rows past the count are zero
    assert not enq["descriptors"][2, cnt[2]:].any()
    for b in (0, 2):
        one = det.run(imgs[b].to(DEV), do_ori=True, desc=net)
        assert torch.equal(one["LAFs"], out[b]["LAFs"])
        assert torch.equal(one["descriptors"], out[b]["descriptors"])


def test_caller_frames(amd, det_nets, net, g, sg, golden_dir):
    """describe_frames on the reference's own graf img1 frames (no shape stage, no orientation: the frames are described as given): 128-D rows,
    source rows by ids[..., 2]; against the reference's descriptors of those frames, and against run()'s rows for the same frames."""
    x = load_gray(os.path.join(golden_dir, "graf_img1.png")).to(DEV)
    frames = torch.from_numpy(sg["LAFs1"]).to(DEV)
    det0 = amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=500, border=5, num_Baum_iters=0).to(DEV)
    d = det0.describe_frames(x, frames, do_ori=False, desc=net)
    src = d["ids"][:, 2].cpu().numpy()
    assert d["descriptors"].shape == (len(src), 128) and len(src) >= 0.99 * 500 and len(set(src.tolist())) == len(src)
    dd = d["descriptors"].cpu().numpy()
    err = float(np.abs(dd - g["desc1"][src]).max())
    r = _extractor(amd, det_nets, 500).run(x, do_ori=True, desc=net)
    gi, wi = match_rows(r["responses"].cpu().numpy(), r["LAFs"].cpu().numpy(), sg["resp1"], sg["LAFs1"])
    pos = {int(s): k for k, s in enumerate(src)}
    keep = [k for k, w in enumerate(wi) if int(w) in pos]
    err_run = float(np.abs(dd[[pos[int(wi[k])] for k in keep]] - r["descriptors"].cpu().numpy()[gi[keep]]).max())
    print("describe_frames on the golden frames: vs the reference's descriptors %.3g, vs run() on %d shared frames %.3g" % (err, len(gi), err_run))
    record_parity("HardTFeat describe_frames on the reference's graf img1 frames", desc_max_abs=err, vs_run_max_abs=err_run, shared_rows=int(len(gi)))
    assert len(gi) >= 0.99 * 500
    # The frames are the reference's own and are described as given, sampled by the project's sampler (the reference's fp32 operation order):
    # what is left is the kernels' distance from the referee plus the reference's, the bar of test_kernel_against_the_referee (2.56e-6; a wrong
    # level or frame moves a patch by >= 7e-3).  run() re-derives the geometry (frames within 1e-3 px): the project's descriptor bar.
    assert err <= (MARGIN + 1.0) * float(g["ref_err_fp64"])
    assert err_run <= DESC_BAR


def test_extractor_arith_governs_the_geometry_only(amd, det_nets, net):
    x = amd.synthetic_image(240, 320, 1).to(DEV)
    det = _extractor(amd, det_nets, 300, arith="fp32_split3")
    r = det.run(x, do_ori=True, desc=net)
    geo = det.run(x, do_ori=True)
    assert torch.equal(geo["LAFs"], r["LAFs"])                                     # the split geometry, with or without the descriptor
    assert torch.equal(r["descriptors"], net(det.extract_patches_from_pyr(r["LAFs"], PS=32)))      # exact fp32 descriptors of that geometry
    from affnet_amd import _lib
    assert det._ctx.arith == _lib.ARITH_FP32_SPLIT3 and net.arith == "fp32"


def test_graf_1_6_matching_end_to_end(amd, det_nets, net, g, sg, golden_dir):
    from affnet_amd import ReprojectionStuff as RS
    det = _extractor(amd, det_nets, 500)
    res, maps, unmatched = [], [], 0
    for k, name in ((1, "graf_img1.png"), (2, "graf_img6.png")):
        r = det.run(load_gray(os.path.join(golden_dir, name)).to(DEV), do_ori=True, desc=net)
        gi, wi = match_rows(r["responses"].cpu().numpy(), r["LAFs"].cpu().numpy(), sg["resp%d" % k], sg["LAFs%d" % k])
        err = float(np.abs(r["descriptors"].cpu().numpy()[gi] - g["desc%d" % k][wi]).max())
        n_rows = int(r["LAFs"].shape[0])
        print("graf image %d: %d rows, %d matched to golden rows, descriptor max abs diff %.3g" % (k, n_rows, len(gi), err))
        record_parity("HardTFeat full path graf img%d vs the reference's golden rows, 500 kp" % (1 if k == 1 else 6), rows=n_rows, matched=int(len(gi)),
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
    record_parity("HardTFeat SNN matching graf 1-6 end to end, 500 kp", tentatives=int(t1.numel()), reference_tentatives=int(len(g["tent1"])),
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
