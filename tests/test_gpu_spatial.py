"""MI355X: spatial verification of tentative matches from their affine frames (csrc/spatial.hip: affnet_verify_score / affnet_verify_matches,
ReprojectionStuff.verify_matches / enqueue_verify / match_and_verify) against the float64 restatement of its rules, tests/_spatial_fp64.py.

The scoring runs in fp32, so a pair whose float64 error lies within BAND = 1e-3 px of the threshold may fall on either side: per hypothesis the
device's count may differ from the float64 count by at most the number of such pairs (rule 1).  Everything after the scoring is exact: the selection
is checked on the device's own counts, the fp64 refit on cases where no pair comes within BAND of the threshold (tests/test_spatial_host.py
asserts that on the CPU), where mask and summary must be identical and the model agree to the project's 1e-3 px bar."""
import os

import numpy as np
import pytest
import torch

import _spatial_fp64 as sp
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TH = 3.0
SENT_I32, SENT_U8 = -7, 0xAB


def raw_verify(l1, l2, tent, count=None, cap=None, th=TH, model=sp.HOMOGRAPHY, lo_iters=3, score_only=False):
    """The C entry point on buffers of this test: counts / inlier are pre-filled with sentinels so that "not written" can be seen.
    -> dict of numpy arrays (counts, inlier, H, summary, best)."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    tent = np.asarray(tent, np.int32).reshape(-1, 2)
    cap = tent.shape[0] if cap is None else cap
    d1, d2 = torch.from_numpy(np.ascontiguousarray(l1, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(l2, np.float32)).to(dev)
    dt = torch.zeros(max(cap, 1), 2, dtype=torch.int32, device=dev)
    dt[:tent.shape[0]] = torch.from_numpy(tent).to(dev)
    dc = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    counts = torch.full((max(cap, 1),), SENT_I32, dtype=torch.int32, device=dev)
    inl = torch.full((max(cap, 1),), SENT_U8, dtype=torch.uint8, device=dev)
    H = torch.full((9,), float("nan"), dtype=torch.float64, device=dev)
    summ = torch.full((4,), SENT_I32, dtype=torch.int32, device=dev)
    best = torch.full((2,), SENT_I32, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.affnet_verify_scratch_bytes(cap), dtype=torch.uint8, device=dev)
    ctx = engine.utility_ctx(dev)
    st = engine.stream_of(dev)
    if score_only:
        check(lib.affnet_verify_score(ctx, ptr(d1), d1.size(0), ptr(d2), d2.size(0), ptr(dt), ptr(dc), cap, th, ptr(counts), ptr(best), ptr(scratch), st), ctx,
              "affnet_verify_score")
    else:
        check(lib.affnet_verify_matches(ctx, ptr(d1), d1.size(0), ptr(d2), d2.size(0), ptr(dt), ptr(dc), cap, th, model, lo_iters, ptr(counts), ptr(H),
                                        ptr(inl), ptr(summ), ptr(scratch), st), ctx, "affnet_verify_matches")
    torch.cuda.synchronize()
    return {"counts": counts.cpu().numpy()[:cap], "inlier": inl.cpu().numpy()[:cap], "H": H.cpu().numpy().reshape(3, 3), "summary": summ.cpu().tolist(),
            "best": best.cpu().tolist()}


_PLANTED = {}


def planted_case(T, seed=0):
    """Planted input + its float64 score, computed once and shared (never modified)."""
    if (T, seed) not in _PLANTED:
        l1, l2, tent, pl = sp.planted(T, seed)
        _PLANTED[(T, seed)] = dict(l1=l1, l2=l2, tent=tent, planted=pl, sc=sp.score(l1, l2, tent, TH))
    return _PLANTED[(T, seed)]


def check_counts(got, sc, what):
    """Rule 1 -> (total |delta|, band share)."""
    got = np.asarray(got, np.int64)
    ok = sc["hyp_ok"]
    delta = np.abs(got - sc["counts"])
    assert (delta[ok] <= sc["band"][ok]).all(), (what, np.nonzero(delta > sc["band"])[0][:8], delta.max())
    assert (got[ok] >= 1).all() and (got[~ok] == 0).all(), what
    return int(delta.sum()), float(sc["band"].sum()) / max(1, got.size ** 2)


def check_select(best, counts_gpu, sc):
    """Rule 2: exact on the device's own counts; the restatement's count of the device's choice is within the two bands of the restatement's maximum."""
    counts_gpu = np.asarray(counts_gpu)
    if counts_gpu.size == 0 or counts_gpu.max() <= 0:
        assert best == -1
        return
    assert best == int(np.argmax(counts_gpu))
    b64 = sp.select(sc["counts"])
    assert sc["counts"][best] >= sc["counts"][b64] - sc["band"][b64] - sc["band"][best]


# the hypothesis tile and the match chunk of the scoring kernel as built (include/affnet_hip.h): one below, at, one above each and twice each
def _edge_sizes():
    from affnet_amd import _lib
    s = {1, 2, 63, 64, 65, 1000}
    for e in (_lib.VERIFY_TILE, _lib.VERIFY_CHUNK):
        s |= {e - 1, e, e + 1, 2 * e - 1, 2 * e, 2 * e + 1}
    return sorted(s)


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000])
def test_counts_and_selection(T):
    assert T in _edge_sizes()
    c = planted_case(T)
    r = raw_verify(c["l1"], c["l2"], c["tent"])
    total, share = check_counts(r["counts"], c["sc"], T)
    check_select(r["summary"][0], r["counts"], c["sc"])
    assert r["summary"][1] == r["counts"].max()
    s = raw_verify(c["l1"], c["l2"], c["tent"], score_only=True)
    assert np.array_equal(s["counts"], r["counts"]) and s["best"] == r["summary"][:2], "the stage entry and the full call score alike"
    again = raw_verify(c["l1"], c["l2"], c["tent"])
    assert np.array_equal(again["counts"], r["counts"]) and np.array_equal(again["H"], r["H"]) and np.array_equal(again["inlier"], r["inlier"]), "same answer every run"
    record_parity("spatial verification counts vs float64, planted T = %d" % T, total_abs_delta=total, band_share=share, band_px=sp.BAND,
                  best=r["summary"][0], best_count=r["summary"][1])


def test_parametrised_sizes_cover_the_built_tile_edges():
    assert _edge_sizes() == [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]


def test_count_pointer_limits_what_is_read_and_written():
    c = planted_case(257)
    ref = raw_verify(c["l1"], c["l2"], c["tent"])
    # capacity 512, 257 valid rows; the rows behind the count point (with valid indices) at frames that are all NaN
    n = c["l1"].shape[0]
    l1 = np.concatenate([c["l1"], np.full((4, 2, 3), np.nan, np.float32)])
    l2 = np.concatenate([c["l2"], np.full((4, 2, 3), np.nan, np.float32)])
    tent = np.concatenate([c["tent"], np.stack([n + np.arange(255) % 4, n + np.arange(255) % 4], 1).astype(np.int32)])
    r = raw_verify(l1, l2, tent, count=257, cap=512)
    assert np.array_equal(r["counts"][:257], ref["counts"]) and (r["counts"][257:] == SENT_I32).all()
    assert np.array_equal(r["inlier"][:257], ref["inlier"]) and (r["inlier"][257:] == SENT_U8).all()
    assert r["summary"] == ref["summary"] and np.array_equal(r["H"], ref["H"])
    # NULL count = count == t_max
    full = raw_verify(c["l1"], c["l2"], c["tent"], count=257, cap=257)
    assert np.array_equal(full["counts"], ref["counts"]) and full["summary"] == ref["summary"] and np.array_equal(full["H"], ref["H"])
    # a count above the capacity is clamped, a count of zero and a capacity of zero give the empty summary
    over = raw_verify(c["l1"], c["l2"], c["tent"], count=100000, cap=257)
    assert np.array_equal(over["counts"], ref["counts"]) and over["summary"] == ref["summary"]
    zero = raw_verify(l1, l2, tent, count=0, cap=512)
    assert zero["summary"] == [-1, 0, 0, 1] and (zero["counts"] == SENT_I32).all() and (zero["inlier"] == SENT_U8).all()
    empty = raw_verify(c["l1"], c["l2"], np.zeros((0, 2), np.int32))
    assert empty["summary"] == [-1, 0, 0, 1] and np.array_equal(empty["H"], np.eye(3))


def test_invalid_hypotheses():
    """A singular L1 (two equal rows), a NaN in L2, an infinite centre: count 0, never best.  All indices are in range (the bounds guard in front of the
    loads is checked by review).  The scoring rule makes a match an inlier when its indices are valid and its centres finite: the row with the infinite
    centre is an inlier of nobody; the rows whose frame SHAPE is unusable keep usable centres and count where the rule says they do - the exact
    six-row case below pins both."""
    c = planted_case(65)
    a, b, tent = c["l1"].copy(), c["l2"].copy(), c["tent"]
    rows = [3, 4, 5]
    a[tent[3, 0], 1, :2] = a[tent[3, 0], 0, :2]
    b[tent[4, 1], 0, 1] = np.nan
    a[tent[5, 0], 0, 2] = np.inf
    sc = sp.score(a, b, tent, TH)
    assert not sc["hyp_ok"][rows].any() and sc["hyp_ok"].sum() == 62
    r = raw_verify(a, b, tent)
    check_counts(r["counts"], sc, "invalid rows")
    check_select(r["summary"][0], r["counts"], sc)
    assert (r["counts"][rows] == 0).all() and r["summary"][0] not in rows
    assert r["inlier"][5] == 0
    # exact: rows 0..2 one valid pair three times, rows 3..5 the same pair through copies of its frames made invalid.  e = 0 for every pair with finite centres.
    i, j = c["tent"][0]
    l1 = np.repeat(c["l1"][i][None], 4, 0)
    l2 = np.repeat(c["l2"][j][None], 4, 0)
    l1[1, 1, :2] = l1[1, 0, :2]          # singular L1
    l2[2, 0, 1] = np.nan                 # NaN in L2
    l1[3, 0, 2] = np.inf                 # infinite centre
    t6 = np.array([[0, 0], [0, 0], [0, 0], [1, 0], [0, 2], [3, 0]], np.int32)
    r = raw_verify(l1, l2, t6, lo_iters=0)
    assert r["counts"].tolist() == [5, 5, 5, 0, 0, 0] and r["summary"] == [0, 5, 5, 0]
    assert r["inlier"].tolist() == [1, 1, 1, 1, 1, 0], "the match with the infinite centre is an inlier of nobody"
    assert r["counts"].tolist() == sp.score(l1, l2, t6, TH)["counts"].tolist()
    # nothing valid: best = -1, flag 1, identity, empty mask
    r = raw_verify(l1, l2, t6[3:])
    assert r["counts"].tolist() == [0, 0, 0] and r["summary"] == [-1, 0, 0, 1] and r["inlier"].tolist() == [0, 0, 0] and np.array_equal(r["H"], np.eye(3))


@pytest.mark.parametrize("model", [sp.HOMOGRAPHY, sp.AFFINE])
def test_degenerate_agreement(model):
    """Every tentative is the same pair: all counts T, best 0, and the refit stops with flag 4 - the masked points of either image coincide, their
    mean distance to the centroid is 0 and no normalisation exists (T >= 4, so the too-few-inliers rule, flag 2, does not trigger first)."""
    c = planted_case(129)
    T = 129
    tent = np.repeat(c["tent"][:1], T, 0)
    r = raw_verify(c["l1"], c["l2"], tent, model=model)
    assert (r["counts"] == T).all() and r["summary"] == [0, T, T, 4] and (r["inlier"] == 1).all()
    assert sp.verify(c["l1"], c["l2"], tent, TH, model, 3)["summary"] == r["summary"]
    assert sp.corner_error(r["H"], sp.hypothesis_model(c["l1"], c["l2"], tent[0])) <= 1e-3


REFIT_CASES = [(65, 0), (65, 1), (65, 2), (65, 3), (257, 0), (257, 1), (257, 2), (257, 3), (1000, 0)]      # tests/test_spatial_host.py: the preconditions hold


@pytest.mark.parametrize("model", [sp.HOMOGRAPHY, sp.AFFINE])
@pytest.mark.parametrize("case", REFIT_CASES)
def test_refit_equals_the_restatement(case, model):
    c = planted_case(*case)
    want = sp.verify(c["l1"], c["l2"], c["tent"], TH, model, 3)
    r = raw_verify(c["l1"], c["l2"], c["tent"], model=model)
    assert np.array_equal(r["inlier"].astype(bool), want["mask"])
    assert r["summary"] == want["summary"], (r["summary"], want["summary"])
    gap = sp.corner_error(r["H"], want["H"])
    print("refit T=%d seed=%d model=%d: corner gap %.3g px, summary %s" % (case[0], case[1], model, gap, r["summary"]))
    assert gap <= 1e-3
    assert r["H"][2, 2] == 1.0 and (model == sp.HOMOGRAPHY or np.array_equal(r["H"][2], [0, 0, 1]))
    if model == sp.HOMOGRAPHY:
        assert np.array_equal(want["mask"], c["planted"])
    # lo_iters = 0: the affine hypothesis and the scoring's own (fp32) inlier set of `best`, which for these cases is the float64 one
    r0 = raw_verify(c["l1"], c["l2"], c["tent"], model=model, lo_iters=0)
    w0 = sp.verify(c["l1"], c["l2"], c["tent"], TH, model, 0)
    assert r0["summary"] == w0["summary"] and np.array_equal(r0["inlier"].astype(bool), w0["mask"])
    gap0 = sp.corner_error(r0["H"], w0["H"])
    assert gap0 <= 1e-3 and np.array_equal(r0["H"][2], [0, 0, 1])
    record_parity("spatial verification refit vs float64, planted T = %d seed %d %s" % (case[0], case[1], "homography" if model else "affine"),
                  corner_gap_px=gap, corner_gap_px_lo0=gap0, inliers=r["summary"][2], best_count=r["summary"][1], bar_px=1e-3)


def test_too_few_inliers_on_real_frames(golden_dir):
    """graf 1-6 at 500 keypoints: 63 tentatives on real detector frames, the best hypothesis has 3 inliers in float64 - a parity leg on realistic
    frame statistics, not a quality claim (that pair has 4 true matches)."""
    g = np.load(os.path.join(golden_dir, "match_graf16_n500.npz"))
    tent = np.stack([g["tent1"], g["tent2"]], 1).astype(np.int32)
    sc = sp.score(g["LAFs1"], g["LAFs2"], tent, TH)
    r = raw_verify(g["LAFs1"], g["LAFs2"], tent)
    total, share = check_counts(r["counts"], sc, "graf")
    check_select(r["summary"][0], r["counts"], sc)
    assert r["summary"][3] == 2 and r["summary"][2] == r["summary"][1] == r["counts"][r["summary"][0]]
    gap = sp.corner_error(r["H"], sp.hypothesis_model(g["LAFs1"], g["LAFs2"], tent[r["summary"][0]]))
    assert gap <= 1e-3 and np.array_equal(r["H"][2], [0, 0, 1])
    assert r["inlier"].sum() == r["summary"][2]
    record_parity("spatial verification on the graf 1-6 golden tentatives (63 rows)", total_abs_delta=total, band_share=share, best_count=r["summary"][1],
                  float64_best_count=int(sc["counts"].max()), corner_gap_px=gap)


def test_match_and_verify_is_match_then_verify_bit_for_bit():
    from affnet_amd import ReprojectionStuff as RS
    T = 300
    c = planted_case(T, 1)
    rng = np.random.default_rng(5)
    d1 = rng.normal(size=(T, 128))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 = rng.normal(size=(T, 128))                           # rows of image 2: outliers keep a random descriptor ...
    src = np.nonzero(c["planted"])[0]
    d2[c["tent"][src, 1]] = d1[src] + 0.02 * rng.normal(size=(len(src), 128))      # ... planted rows a noisy copy, at the shuffled position of their frame
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    dev = torch.device(DEV)
    D1, D2 = torch.from_numpy(d1.astype(np.float32)).to(dev), torch.from_numpy(d2.astype(np.float32)).to(dev)
    L1, L2 = torch.from_numpy(c["l1"]).to(dev), torch.from_numpy(c["l2"]).to(dev)
    for model in ("homography", "affine"):
        t1, t2, H, inl, info = RS.match_and_verify(D1, D2, L1, L2, 0.8, TH, model, 3)
        m1, m2, _, _ = RS.match_snn(D1, D2, 0.8)
        H2, inl2, info2 = RS.verify_matches(L1, L2, m1, m2, TH, model, 3)
        assert torch.equal(t1, m1) and torch.equal(t2, m2) and len(src) <= t1.numel() < T
        assert torch.equal(H, H2) and torch.equal(inl, inl2) and inl.dtype == torch.bool and H.dtype == torch.float64 and H.shape == (3, 3)
        assert torch.equal(info["counts"], info2["counts"])
        assert {k: v for k, v in info.items() if k != "counts"} == {k: v for k, v in info2.items() if k != "counts"}
        assert info["flags"] == 0 and info["num_inliers"] == int(inl.sum()) >= info["best_count"] >= 1
        if model == "homography":        # every planted row was matched and verified
            got = set(zip(t1[inl].tolist(), t2[inl].tolist()))
            assert got >= set(zip(src.tolist(), c["tent"][src, 1].tolist()))
    assert RS.verify_matches(L1, L2, m1[:0], m2[:0])[2]["flags"] == 1


def test_end_to_end_on_a_warped_image(weights):
    """synthetic_image(240, 320) and its warp under the planted H scaled to that size; 300 keypoints, AffNet + OriNet + the synthetic HardNet,
    match_and_verify.  Asserted: parity with the restatement on the same tentatives (rules 1 and 2; the refit rule where its precondition holds for
    this input, said in the parity report).  Recorded, not asserted: inlier count and corner error against the planted H."""
    import affnet_amd
    from affnet_amd import ReprojectionStuff as RS
    dev = torch.device(DEV)
    h, w = 240, 320
    S = np.diag([w / 1000.0, w / 1000.0, 1.0])
    Hs = S @ sp.PLANTED_H @ np.linalg.inv(S)
    Hs /= Hs[2, 2]
    img1 = affnet_amd.synthetic_image(h, w, 3).to(dev)
    Hi = torch.from_numpy(np.linalg.inv(Hs)).to(dev)
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float64), torch.arange(w, device=dev, dtype=torch.float64), indexing="ij")
    src = torch.stack([xs, ys, torch.ones_like(xs)], -1) @ Hi.T
    sx, sy = src[..., 0] / src[..., 2], src[..., 1] / src[..., 2]
    grid = torch.stack([(2 * sx + 1) / w - 1, (2 * sy + 1) / h - 1], -1).float()[None]
    img2 = torch.nn.functional.grid_sample(img1, grid, mode="bilinear", padding_mode="zeros", align_corners=False).contiguous()
    A = affnet_amd.AffNetFast(PS=32); A.load_state_dict(weights["AffNet"]); A.to(dev)
    O = affnet_amd.OriNetFast(PS=32); O.load_state_dict(weights["OriNet"]); O.to(dev)
    Hn = affnet_amd.HardNet(); Hn.load_state_dict(weights["HardNet"]); Hn.to(dev)
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=300, border=5, num_Baum_iters=1, AffNet=A, OriNet=O).to(dev)
    r1, r2 = det.run_batch(torch.cat([img1, img2], 0), do_ori=True, desc=Hn)
    t1, t2, H, inl, info = RS.match_and_verify(r1["descriptors"], r2["descriptors"], r1["LAFs"], r2["LAFs"], 0.8, TH, "homography", 3)
    l1, l2 = r1["LAFs"].cpu().numpy(), r2["LAFs"].cpu().numpy()
    tent = np.stack([t1.cpu().numpy(), t2.cpu().numpy()], 1).astype(np.int32)
    T = tent.shape[0]
    assert info["counts"].numel() == T
    sc = sp.score(l1, l2, tent, TH)
    counts = info["counts"].cpu().numpy()
    total, share = check_counts(counts, sc, "end to end")
    check_select(info["best"], counts, sc)
    assert info["best_count"] == (counts.max() if T else 0) and info["num_inliers"] == int(inl.sum())
    # rule 6 where its precondition holds: same hypothesis and start set as in float64, no pair within BAND of the threshold in any refit
    want = sp.verify(l1, l2, tent, TH, sp.HOMOGRAPHY, 3)
    refit_checked = bool(want["best"] == info["best"] and sc["band"][want["best"]] == 0 and want["margin"] > sp.BAND)
    gap = float("nan")
    if refit_checked:
        assert np.array_equal(inl.cpu().numpy(), want["mask"])
        assert [info["best"], info["best_count"], info["num_inliers"], info["flags"]] == want["summary"]
        gap = sp.corner_error(H.cpu().numpy(), want["H"])
        assert gap <= 1e-3
    corners = np.array([[0.0, 0.0], [w, 0.0], [w, h], [0.0, h]])
    record_parity("spatial verification end to end, synthetic 320x240 pair under the planted H, 300 kp", tentatives=T, inliers=info["num_inliers"],
                  best_count=info["best_count"], flags=info["flags"], corner_error_vs_planted_px=sp.corner_error(H.cpu().numpy(), Hs, corners),
                  total_abs_delta=total, band_share=share, refit_rule_checked=refit_checked, corner_gap_vs_float64_px=gap)
