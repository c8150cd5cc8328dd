"""MI355X: epipolar verification of tentative matches from their affine frames (csrc/epipolar.hip: affnet_epipolar_score / affnet_epipolar_verify,
ReprojectionStuff.verify_epipolar / enqueue_verify_epipolar / model="fundamental") against the restatement of its rules, tests/_epipolar_fp64.py.

The hypotheses are compared through what they are for, the Sampson distances they give; the fp32 scoring and the selection are exact on the device's
own hypotheses; the fp64 refit is held against the restatement's refit from the device's own start mask."""
import numpy as np
import pytest
import torch

import _epipolar_fp64 as ep
import _spatial_fp64 as sp
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TH, ROUNDS = 2.0, 8
SENT_I32, SENT_U8, SENT_F32 = -7, 0xAB, -12345.0
# px: ten times the largest difference between the fp64 Sampson distances (below 10 px) under the restatement's float64 F and under the same F rounded
# to float32, MEASURED on the CPU over all valid hypotheses x all matches of the 18 inputs of test_hypotheses_match_the_restatement (seed 0): the
# largest difference was 6.21e-3 px (T = 128, rounds = 8); ten times that, rounded up to two digits.
HYP_BAR = 6.3e-2
REFIT_BAR = 1e-6
SIZES, ROUND_CASES = [3, 8, 63, 64, 65, 127, 128, 129, 257], [1, 8]


def raw_epi(l1, l2, tent, count=None, cap=None, th=TH, rounds=ROUNDS, seed=0, lo_iters=3, score_only=False):
    """The C entry points on buffers of this test, pre-filled with sentinels so that "not written" can be seen -> dict of numpy arrays."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    tent = np.asarray(tent, np.int32).reshape(-1, 2)
    cap = tent.shape[0] if cap is None else cap
    d1, d2 = torch.from_numpy(np.ascontiguousarray(l1, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(l2, np.float32)).to(dev)
    dt = torch.zeros(max(cap, 1), 2, dtype=torch.int32, device=dev)
    dt[:tent.shape[0]] = torch.from_numpy(tent).to(dev)
    dc = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    nh = max(cap * rounds, 1)
    hyp = torch.full((nh, 9), SENT_F32, dtype=torch.float32, device=dev)
    counts = torch.full((nh,), SENT_I32, dtype=torch.int32, device=dev)
    inl = torch.full((max(cap, 1),), SENT_U8, dtype=torch.uint8, device=dev)
    F = torch.full((9,), float("nan"), dtype=torch.float64, device=dev)
    summ = torch.full((4,), SENT_I32, dtype=torch.int32, device=dev)
    best = torch.full((2,), SENT_I32, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.affnet_epipolar_scratch_bytes(cap, rounds), dtype=torch.uint8, device=dev)
    ctx = engine.utility_ctx(dev)
    st = engine.stream_of(dev)
    if score_only:
        check(lib.affnet_epipolar_score(ctx, ptr(d1), d1.size(0), ptr(d2), d2.size(0), ptr(dt), ptr(dc), cap, th, rounds, seed, ptr(hyp), ptr(counts), ptr(best),
                                        ptr(scratch), st), ctx, "affnet_epipolar_score")
    else:
        check(lib.affnet_epipolar_verify(ctx, ptr(d1), d1.size(0), ptr(d2), d2.size(0), ptr(dt), ptr(dc), cap, th, rounds, seed, lo_iters, ptr(counts), ptr(F),
                                         ptr(inl), ptr(summ), ptr(scratch), st), ctx, "affnet_epipolar_verify")
    torch.cuda.synchronize()
    return {"hyp": hyp.cpu().numpy()[:cap * rounds], "counts": counts.cpu().numpy()[:cap * rounds], "inlier": inl.cpu().numpy()[:cap], "F": F.cpu().numpy(),
            "summary": summ.cpu().tolist(), "best": best.cpu().tolist()}


_CASES = {}


def depth_case(T, share=0.5, seed=None):
    """Planted scene with depth, computed once and shared (never modified)."""
    seed = T if seed is None else seed
    if (T, share, seed) not in _CASES:
        l1, l2, tent, pl, F = ep.planted_two_view(T, share, seed)
        _CASES[(T, share, seed)] = dict(l1=l1, l2=l2, tent=tent, planted=pl, F=F)
    return _CASES[(T, share, seed)]


def check_score(s, pts, th=TH):
    """counts and best are the fp32 scoring mirror fed with the device's own hypotheses, bit for bit -> the mirror's inlier matrix."""
    counts, inl, _ = ep.score_fp32(s["hyp"], pts, th)
    assert np.array_equal(s["counts"], counts), np.nonzero(s["counts"] != counts)[0][:8]
    b = sp.select(counts)
    assert s["best"] == [b, int(counts[b]) if b >= 0 else 0]
    return inl


def check_hyp(s, hy, what):
    """validity exactly, valid models through their Sampson distances -> the largest difference (px)."""
    valid = np.isfinite(s["hyp"]).all(1)
    assert np.array_equal(valid, hy["ok"]), (what, np.nonzero(valid != hy["ok"])[0][:8])
    assert np.isnan(s["hyp"][~valid]).all() and (s["counts"][~valid] == 0).all(), what
    if not valid.any():
        return 0.0
    got, want = ep.sampson(s["hyp"][valid].astype(np.float64), hy["pts"]), ep.sampson(hy["F"][valid], hy["pts"])
    with np.errstate(all="ignore"):
        near = want < 10.0
        gap = float(np.abs(got - want)[near].max()) if near.any() else 0.0
    assert gap <= HYP_BAR, (what, gap)
    return gap


@pytest.mark.parametrize("rounds", ROUND_CASES)
@pytest.mark.parametrize("T", SIZES)
def test_hypotheses_match_the_restatement(T, rounds):
    c = depth_case(T)
    hy = ep.hypotheses(c["l1"], c["l2"], c["tent"], rounds, 0)
    s = raw_epi(c["l1"], c["l2"], c["tent"], rounds=rounds, score_only=True)
    assert hy["ok"].all(), "every hypothesis of a scene of sound frames is valid"
    gap = check_hyp(s, hy, (T, rounds))
    n2 = (s["hyp"].astype(np.float64) ** 2).sum(1)
    assert np.abs(n2 - 1.0).max() < 1e-6 and (np.abs(s["hyp"]).max(1) == s["hyp"].max(1)).all(), "unit norm, largest entry positive"
    check_score(s, hy["pts"])
    same = float((s["hyp"] == hy["hyp32"]).all(1).mean())
    print("T=%d rounds=%d: Sampson gap %.3g px (bar %.3g), hypotheses equal to the restatement's float32 bit for bit: %.4f" % (T, rounds, gap, HYP_BAR, same))
    v = raw_epi(c["l1"], c["l2"], c["tent"], rounds=rounds)
    assert np.array_equal(v["counts"], s["counts"]) and v["summary"][:2] == s["best"], "the stage entry and the full call score alike"
    record_parity("epipolar hypotheses vs float64, depth scene T = %d rounds = %d" % (T, rounds), sampson_gap_px=gap, bar_px=HYP_BAR, bit_equal_share=same,
                  best=s["best"][0], best_count=s["best"][1])


def test_parametrised_sizes_cover_the_built_tile_edges():
    """T crosses the match chunk and the solve tile, T * rounds the scoring tile and the solve tile: one below, at and one above each, with rounds = 1 for
    T itself and rounds = 8 for a product; T = 3 is the smallest valid input, 257 more than two chunks."""
    from affnet_amd import _lib
    assert (_lib.EPI_TILE, _lib.EPI_CHUNK, _lib.EPI_SOLVE_TILE) == (128, 128, 64)
    for e in (_lib.EPI_CHUNK, _lib.EPI_SOLVE_TILE):
        assert {e - 1, e, e + 1} <= set(SIZES)
    prods = {T * r for T in SIZES for r in ROUND_CASES}
    for e in (_lib.EPI_TILE, _lib.EPI_SOLVE_TILE):
        assert {e - 1, e, e + 1} <= prods and any(p > 2 * e and p % e for p in prods) and any(p > 2 * e and p % e == 0 for p in prods)
    assert 3 in SIZES and max(SIZES) > 2 * _lib.EPI_CHUNK and 1 in ROUND_CASES


def test_count_pointer_limits_what_is_read_and_written():
    c = depth_case(257)
    ref = raw_epi(c["l1"], c["l2"], c["tent"])
    ref_s = raw_epi(c["l1"], c["l2"], c["tent"], score_only=True)
    # capacity 512, 257 valid rows; the rows behind the count point (with valid indices) at frames that are all NaN
    n = c["l1"].shape[0]
    l1 = np.concatenate([c["l1"], np.full((4, 2, 3), np.nan, np.float32)])
    l2 = np.concatenate([c["l2"], np.full((4, 2, 3), np.nan, np.float32)])
    tent = np.concatenate([c["tent"], np.stack([n + np.arange(255) % 4, n + np.arange(255) % 4], 1).astype(np.int32)])
    r = raw_epi(l1, l2, tent, count=257, cap=512)
    nh = 257 * ROUNDS
    assert np.array_equal(r["counts"][:nh], ref["counts"]) and (r["counts"][nh:] == SENT_I32).all()
    assert np.array_equal(r["inlier"][:257], ref["inlier"]) and (r["inlier"][257:] == SENT_U8).all()
    assert r["summary"] == ref["summary"] and np.array_equal(r["F"], ref["F"])
    s = raw_epi(l1, l2, tent, count=257, cap=512, score_only=True)
    assert np.array_equal(s["hyp"][:nh], ref_s["hyp"]) and (s["hyp"][nh:] == SENT_F32).all() and (s["counts"][nh:] == SENT_I32).all()
    assert np.array_equal(s["counts"][:nh], ref_s["counts"]) and s["best"] == ref_s["best"]
    # NULL count = count == t_max; a count above the capacity is clamped
    full = raw_epi(c["l1"], c["l2"], c["tent"], count=257, cap=257)
    over = raw_epi(c["l1"], c["l2"], c["tent"], count=100000, cap=257)
    for x in (full, over):
        assert np.array_equal(x["counts"], ref["counts"]) and x["summary"] == ref["summary"] and np.array_equal(x["F"], ref["F"])
    # a count of zero and a capacity of zero give the empty summary and the zero model
    zero = raw_epi(l1, l2, tent, count=0, cap=512)
    assert zero["summary"] == [-1, 0, 0, 1] and (zero["counts"] == SENT_I32).all() and (zero["inlier"] == SENT_U8).all() and not zero["F"].any()
    zs = raw_epi(l1, l2, tent, count=0, cap=512, score_only=True)
    assert zs["best"] == [-1, 0] and (zs["hyp"] == SENT_F32).all() and (zs["counts"] == SENT_I32).all()
    empty = raw_epi(c["l1"], c["l2"], np.zeros((0, 2), np.int32))
    assert empty["summary"] == [-1, 0, 0, 1] and not empty["F"].any()


def _compare_invalid(l1, l2, tent, what):
    hy = ep.hypotheses(l1, l2, tent, ROUNDS, 0)
    s = raw_epi(l1, l2, tent, score_only=True)
    check_hyp(s, hy, what)
    inl = check_score(s, hy["pts"])
    assert not inl[:, ~hy["match_ok"]].any(), what
    return hy, s, inl


def test_invalid_input():
    c = depth_case(65)
    tent = c["tent"]
    # out-of-range indices (never loaded through), NaN / inf in a frame
    a, b, t2 = c["l1"].copy(), c["l2"].copy(), tent.copy()
    b[tent[4, 1], 0, 1] = np.nan                  # a shape number: no member, but usable centres
    a[tent[5, 0], 0, 2] = np.inf                  # a centre: no member, no match
    t2[6], t2[7], t2[8] = (-1, 0), (0, len(b)), (2 ** 31 - 1, -2 ** 31)
    hy, s, inl = _compare_invalid(a, b, t2, "bad rows")
    bad = np.isin(hy["mem"], [4, 5, 6, 7, 8]).any(1)
    assert np.array_equal(~hy["ok"], bad) and hy["match_ok"][4] and not hy["match_ok"][[5, 6, 7, 8]].any()
    # ... and the result otherwise ignores those rows: the hypotheses without them are those of the clean input, their inliers differ only in the bad rows
    clean = raw_epi(c["l1"], c["l2"], tent, score_only=True)
    assert np.array_equal(s["hyp"][~bad], clean["hyp"][~bad])
    inl_clean = ep.score_fp32(clean["hyp"], ep.gather(c["l1"], c["l2"], tent)[0], TH)[1]
    keep = np.ones(65, bool)
    keep[[4, 5, 6, 7, 8]] = False
    assert np.array_equal(inl[~bad][:, keep], inl_clean[~bad][:, keep])
    v = raw_epi(a, b, t2)
    assert v["summary"][0] >= 0 and not bad[v["summary"][0]] and not v["inlier"][[5, 6, 7, 8]].any()
    # T of 1 and 2: nothing valid, flag 1, zero model, empty mask
    for T in (1, 2):
        hy, s, _ = _compare_invalid(c["l1"], c["l2"], tent[:T], "T = %d" % T)
        assert not hy["ok"].any() and s["best"] == [-1, 0]
        v = raw_epi(c["l1"], c["l2"], tent[:T])
        assert v["summary"] == [-1, 0, 0, 1] and not v["F"].any() and not v["inlier"].any() and not v["counts"].any()
    # a singular frame among the members: zero size in both images (three coincident correspondences: invalid), and a rank-1 shape in image 1 only
    z1, z2 = c["l1"].copy(), c["l2"].copy()
    z1[tent[9, 0], :, :2] = 0.0
    z2[tent[9, 1], :, :2] = 0.0
    z1[tent[10, 0], 1, :2] = z1[tent[10, 0], 0, :2]
    hy, s, _ = _compare_invalid(z1, z2, tent, "singular frames")
    with9 = (hy["mem"] == 9).any(1)
    assert with9.any() and not hy["ok"][with9].any() and hy["match_ok"].all()


@pytest.mark.parametrize("case", [(257, 0.5, None), (129, 0.5, None), (200, 0.5, 7)])
def test_refit_equals_the_restatement(case):
    c = depth_case(*case)
    pts = ep.gather(c["l1"], c["l2"], c["tent"])[0]
    s = raw_epi(c["l1"], c["l2"], c["tent"], score_only=True)
    inl = check_score(s, pts)
    b = s["best"][0]
    # lo_iters = 0: model 0 is the stored hypothesis widened to double, its mask the scoring kernel's own inlier set
    r0 = raw_epi(c["l1"], c["l2"], c["tent"], lo_iters=0)
    assert np.array_equal(r0["F"], s["hyp"][b].astype(np.float64)) and np.array_equal(r0["inlier"].astype(bool), inl[b])
    assert r0["summary"] == [b, s["best"][1], s["best"][1], 0]
    for it in (1, 3):
        r = raw_epi(c["l1"], c["l2"], c["tent"], lo_iters=it)
        want = ep.refine(pts, s["hyp"][b].astype(np.float64), inl[b], TH, it, b, s["best"][1])
        assert r["summary"] == want["summary"], (r["summary"], want["summary"])
        if want["margin"] > REFIT_BAR:
            assert np.array_equal(r["inlier"].astype(bool), want["mask"])
        m = want["mask"]
        gap = float(np.abs(ep.sampson(r["F"], pts) - ep.sampson(want["F"], pts))[m].max())
        print("refit %s lo_iters=%d: summary %s, margin %.3g px, Sampson gap on the mask %.3g px" % (case, it, r["summary"], want["margin"], gap))
        assert gap <= REFIT_BAR
        F = r["F"].reshape(3, 3)
        assert abs((F * F).sum() - 1.0) < 1e-12 and F.flat[np.argmax(np.abs(F))] > 0
        assert r["summary"][2] > r["summary"][1] and np.linalg.svd(F, compute_uv=False)[2] < 1e-9, "a refit won, and a refitted model has rank 2"
        record_parity("epipolar refit vs float64, depth scene %s lo_iters %d" % (case, it), sampson_gap_px=gap, margin_px=want["margin"], inliers=r["summary"][2],
                      best_count=r["summary"][1], bar_px=REFIT_BAR)


def test_refit_flags():
    for rows, flag in ((ep.few_rows, 2), (ep.collinear_rows, 4)):
        l1, l2, tent = rows()
        r = raw_epi(l1, l2, tent)
        s = raw_epi(l1, l2, tent, score_only=True)
        pts = ep.gather(l1, l2, tent)[0]
        inl = check_score(s, pts)
        b = s["best"][0]
        want = ep.refine(pts, s["hyp"][b].astype(np.float64), inl[b], TH, 3, b, s["best"][1])
        assert r["summary"][3] == flag and r["summary"] == want["summary"] and r["summary"] == ep.verify(l1, l2, tent, TH, ROUNDS, 0, 3)["summary"]
        assert (r["summary"][1] <= 5) if flag == 2 else (r["summary"][1] >= 8)
        assert np.array_equal(r["F"], s["hyp"][b].astype(np.float64)) and np.array_equal(r["inlier"].astype(bool), inl[b]), "model 0 and its mask stay"


@pytest.mark.parametrize("scene", ep.SCENES + ep.PLANAR)
def test_planted_recovery_on_the_device(scene):
    if len(scene) == 3:
        l1, l2, tent, _, F = ep.planted_two_view(*scene)
        gt = ep.sampson(F.reshape(9), ep.gather(l1, l2, tent)[0]) <= TH
    else:
        l1, l2, tent, gt = sp.planted(*scene)
    r = raw_epi(l1, l2, tent)
    want = ep.verify(l1, l2, tent, TH, ROUNDS, 0, 3)
    mask = r["inlier"].astype(bool)
    kept, others = int((mask & gt).sum()), int((mask & ~gt).sum())
    print("scene %s: summary %s (restatement %s), kept %d of %d, others %d" % (scene, r["summary"], want["summary"], kept, gt.sum(), others))
    assert r["summary"][3] == 0 and r["summary"][2] == mask.sum()
    assert kept >= 0.95 * gt.sum(), (kept, gt.sum())
    if len(scene) == 3:
        assert others <= 0.05 * gt.sum(), (others, gt.sum())
    diff = mask != want["mask"]
    assert not (diff & ~want["near"]).any(), np.nonzero(diff & ~want["near"])[0]
    record_parity("epipolar verification, planted scene %s" % (scene,), kept=kept, ground_truth=int(gt.sum()), others=others, differs_from_restatement=int(diff.sum()),
                  band_px=ep.BAND, best_count=r["summary"][1])


def _descriptors(c, T):
    rng = np.random.default_rng(5)
    d1 = rng.normal(size=(T, 128))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 = rng.normal(size=(T, 128))                           # rows of image 2: outliers keep a random descriptor ...
    src = np.nonzero(c["planted"])[0]
    d2[c["tent"][src, 1]] = d1[src] + 0.02 * rng.normal(size=(len(src), 128))      # ... planted rows a noisy copy, at the shuffled position of their frame
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    dev = torch.device(DEV)
    return torch.from_numpy(d1.astype(np.float32)).to(dev), torch.from_numpy(d2.astype(np.float32)).to(dev), src


def test_determinism_and_the_chain():
    from affnet_amd import ReprojectionStuff as RS
    scene = (200, 0.5, 7)
    c = depth_case(*scene)
    a, b = raw_epi(c["l1"], c["l2"], c["tent"]), raw_epi(c["l1"], c["l2"], c["tent"])
    sa, sb = raw_epi(c["l1"], c["l2"], c["tent"], score_only=True), raw_epi(c["l1"], c["l2"], c["tent"], score_only=True)
    for x, y in ((a, b), (sa, sb)):
        assert all(np.array_equal(x[k], y[k], equal_nan=True) for k in ("hyp", "counts", "inlier", "F")) and x["summary"] == y["summary"] and x["best"] == y["best"]
    # another seed: other hypotheses, the same final mask outside BAND
    o = raw_epi(c["l1"], c["l2"], c["tent"], seed=1)
    assert not np.array_equal(o["counts"], a["counts"])
    near = ep.verify(c["l1"], c["l2"], c["tent"], TH, ROUNDS, 0, 3)["near"] | ep.verify(c["l1"], c["l2"], c["tent"], TH, ROUNDS, 1, 3)["near"]
    assert not ((o["inlier"] != a["inlier"]) & ~near).any()
    # the chain: match_and_verify(model="fundamental") = match_snn, then verify_epipolar (= verify_matches(model="fundamental")), bit for bit
    dev = torch.device(DEV)
    T = 200
    D1, D2, src = _descriptors(c, T)
    L1, L2 = torch.from_numpy(c["l1"]).to(dev), torch.from_numpy(c["l2"]).to(dev)
    t1, t2, F, inl, info = RS.match_and_verify(D1, D2, L1, L2, 0.8, TH, "fundamental", 3, rounds=ROUNDS, seed=3)
    m1, m2, _, _ = RS.match_snn(D1, D2, 0.8)
    F2, inl2, info2 = RS.verify_epipolar(L1, L2, m1, m2, TH, ROUNDS, 3, 3)
    F3, inl3, info3 = RS.verify_matches(L1, L2, m1, m2, TH, "fundamental", 3, rounds=ROUNDS, seed=3)
    assert torch.equal(t1, m1) and torch.equal(t2, m2) and len(src) <= t1.numel() < T
    for Fx, inlx, infox in ((F2, inl2, info2), (F3, inl3, info3)):
        assert torch.equal(F, Fx) and torch.equal(inl, inlx) and inl.dtype == torch.bool and F.dtype == torch.float64 and F.shape == (3, 3)
        assert torch.equal(info["counts"], infox["counts"]) and info["counts"].numel() == t1.numel() * ROUNDS
        assert {k: v for k, v in info.items() if k != "counts"} == {k: v for k, v in infox.items() if k != "counts"}
    assert set(info) == {"counts", "best", "best_count", "num_inliers", "flags", "rounds", "seed"} and info["rounds"] == ROUNDS and info["seed"] == 3
    assert info["flags"] == 0 and info["num_inliers"] == int(inl.sum()) >= info["best_count"] >= 8
    # the Python result is the C entry point's on the same tentatives, and sampson_distance is the restatement's distance
    tent = np.stack([m1.cpu().numpy(), m2.cpu().numpy()], 1).astype(np.int32)
    raw = raw_epi(c["l1"], c["l2"], tent, seed=3)
    assert np.array_equal(raw["F"].reshape(3, 3), F.cpu().numpy()) and np.array_equal(raw["inlier"].astype(bool), inl.cpu().numpy())
    d = RS.sampson_distance(F, L1, L2, m1, m2).cpu().numpy()
    want = ep.sampson(F.cpu().numpy().reshape(9), ep.gather(c["l1"], c["l2"], tent)[0])
    assert d.dtype == np.float64 and np.allclose(d, want, rtol=1e-9, atol=1e-9)
    assert np.array_equal(d <= TH, inl.cpu().numpy()) or np.abs(d - TH).min() < 1e-9
    assert RS.verify_epipolar(L1, L2, m1[:0], m2[:0])[2]["flags"] == 1


def test_planar_models_through_the_same_functions_are_unchanged():
    """model='homography' / 'affine' through verify_matches / match_and_verify, with and without the new keyword arguments: the bytes of
    affnet_verify_matches called directly."""
    from affnet_amd import ReprojectionStuff as RS
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    T = 300
    l1, l2, tent, pl = sp.planted(T, 1)
    c = dict(l1=l1, l2=l2, tent=tent, planted=pl)
    D1, D2, src = _descriptors(c, T)
    L1, L2 = torch.from_numpy(l1).to(dev), torch.from_numpy(l2).to(dev)
    m1, m2, _, _ = RS.match_snn(D1, D2, 0.8)
    k = m1.numel()
    dt = torch.stack([m1, m2], 1).to(torch.int32).contiguous()
    for model, code in (("homography", 1), ("affine", 0)):
        counts = torch.zeros(k, dtype=torch.int32, device=dev)
        H = torch.zeros(3, 3, dtype=torch.float64, device=dev)
        inl = torch.zeros(k, dtype=torch.uint8, device=dev)
        summ = torch.zeros(4, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.affnet_verify_scratch_bytes(k), dtype=torch.uint8, device=dev)
        ctx = engine.utility_ctx(dev)
        check(lib.affnet_verify_matches(ctx, ptr(L1), T, ptr(L2), T, ptr(dt), None, k, 3.0, code, 3, ptr(counts), ptr(H), ptr(inl), ptr(summ), ptr(scratch),
                                        engine.stream_of(dev)), ctx, "affnet_verify_matches")
        torch.cuda.synchronize()
        for kw in ({}, dict(rounds=32, seed=9)):
            H1, inl1, info1 = RS.verify_matches(L1, L2, m1, m2, 3.0, model, 3, **kw)
            t1, t2, H2, inl2, info2 = RS.match_and_verify(D1, D2, L1, L2, 0.8, 3.0, model, 3, **kw)
            assert torch.equal(t1, m1) and torch.equal(t2, m2)
            for Hx, inlx, infox in ((H1, inl1, info1), (H2, inl2, info2)):
                assert torch.equal(Hx, H) and torch.equal(inlx, inl.bool()) and torch.equal(infox["counts"], counts)
                assert [infox["best"], infox["best_count"], infox["num_inliers"], infox["flags"]] == summ.cpu().tolist()
                assert set(infox) == {"counts", "best", "best_count", "num_inliers", "flags"}
        assert H[2, 2] == 1.0 and (model == "affine" or int(inl.sum()) >= len(src)), "the homography keeps every planted row of this planar scene"
