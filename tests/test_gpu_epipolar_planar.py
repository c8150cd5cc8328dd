"""MI355X: plane-aware epipolar verification (csrc/epipolar_planar.hip: affnet_epipolar_planar_score / affnet_epipolar_verify_planar,
ReprojectionStuff.verify_epipolar_planar / enqueue_verify_epipolar_planar / model="fundamental_planar") against the restatement of its rules,
tests/_epipolar_planar_fp64.py.

The plane and the plain F are the bytes of the two calls this one contains; the off-plane list, the fp32 scoring and the selection are exact
given the device's own plane mask and hypotheses; the hypotheses and the refit are compared through the Sampson distances they give."""
import numpy as np
import pytest
import torch

import _epipolar_fp64 as ep
import _epipolar_planar_fp64 as pp
import _spatial_fp64 as sp
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TH, PLANE_TH, ROUNDS = 2.0, 3.0, 8
SENT_I32, SENT_U8, SENT_F32 = -7, 0xAB, -12345.0
# px: ten times the largest difference between the fp64 Sampson distances (below 10 px) under the restatement's float64 F and under the same F
# rounded to float32, MEASURED on the CPU with the restatement (its own plane) over all valid hypotheses x all matches of the inputs check_stages
# sees here - the 20 of SIZE_CASES, the two DEGENERATE scenes, scene (64, 40, 8, 1) at rounds = 8 (also at inl_th = 0.01), the seven of
# pp.REFIT_SCENES at rounds = 1 and the two outlier sets, seed 0, lo_iters 3: the largest difference was 5.46e-3 px (scene (129, 80, 12, 21), rounds = 1;
# 1.69e-3 px over SIZE_CASES, at T = 128, rounds = 8); ten times that, rounded up to two digits.
HYP_BAR = 5.5e-2
# px: the same measurement for the refitted models: ten times the largest difference between the fp64 Sampson distances (below 10 px) under the
# restatement's kept float64 F and under that F rounded to float32, MEASURED on the CPU over the seven inputs of pp.REFIT_SCENES (rounds = 1): the
# largest difference was 3.43e-5 px (scene (129, 80, 12, 21)); ten times that, rounded up to two digits.
REFIT_BAR = 3.5e-4
SIZES, ROUND_CASES = [3, 8, 63, 64, 65, 127, 128, 129, 257], [1, 8]
# T -> (matches on the plane, off the plane, scene seed, U): the rest of the T rows are random outliers, which are off the plane too.  Found by
# a search on the CPU with the restatement: U is what its plane stage leaves, with no match within 1e-2 px of plane_th in its refits.
SCENE_OF = {3: (1, 2, 1, 2), 8: (6, 2, 1, 6), 63: (55, 8, 1, 8), 64: (48, 16, 1, 16), 65: (57, 8, 1, 8), 127: (64, 63, 1, 63), 128: (64, 61, 1, 64),
            129: (64, 65, 2, 65), 257: (129, 128, 57, 128)}
EXTRA = [(257, 1, (130, 127, 57, 127)), (257, 1, (128, 129, 57, 129))]        # U one below and one above the scoring tile
SIZE_CASES = [(T, r, SCENE_OF[T]) for T in SIZES for r in ROUND_CASES] + EXTRA
DEGENERATE = [(200, 120, 16, 5), (128, 90, 6, 6)]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def raw(l1, l2, tent, what, count=None, cap=None, th=TH, plane_th=PLANE_TH, rounds=ROUNDS, seed=0, lo_iters=3, scratch_fill=None):
    """The C entry points on buffers of this test, pre-filled with sentinels so that "not written" can be seen -> dict of numpy arrays.
    what: 'planar', 'planar_score', 'plain' (affnet_epipolar_verify) or 'plane' (affnet_verify_matches, homography, plane_th)."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    tent = np.asarray(tent, np.int32).reshape(-1, 2)
    cap = tent.shape[0] if cap is None else cap
    d1, d2 = _dev(l1, np.float32), _dev(l2, np.float32)
    dt = torch.zeros(max(cap, 1), 2, dtype=torch.int32, device=dev)
    dt[:tent.shape[0]] = torch.from_numpy(tent).to(dev)
    dc = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    nh, n = max(cap * rounds, 1), max(cap, 1)
    i32 = lambda *s: torch.full(s, SENT_I32, dtype=torch.int32, device=dev)
    u8 = lambda *s: torch.full(s, SENT_U8, dtype=torch.uint8, device=dev)
    f64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    hyp = torch.full((nh, 9), SENT_F32, dtype=torch.float32, device=dev)
    o = dict(counts=i32(nh), inlier=u8(n), F=f64(9), summary=i32(4), H=f64(9), plane_inlier=u8(n), plane_summary=i32(4), info=i32(4), list=i32(n), n_off=i32(2),
             best=i32(2), plane_counts=i32(n))
    size = {"planar": lib.affnet_epipolar_planar_scratch_bytes, "planar_score": lib.affnet_epipolar_planar_scratch_bytes,
            "plain": lib.affnet_epipolar_scratch_bytes}
    nbytes = lib.affnet_verify_scratch_bytes(cap) if what == "plane" else size[what](cap, rounds)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if scratch_fill is None else torch.full((nbytes,), scratch_fill, dtype=torch.uint8, device=dev)
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    head = (ctx, ptr(d1), d1.size(0), ptr(d2), d2.size(0), ptr(dt), ptr(dc), cap)
    if what == "planar":
        rc = lib.affnet_epipolar_verify_planar(*head, th, plane_th, rounds, seed, lo_iters, ptr(o["counts"]), ptr(o["F"]), ptr(o["inlier"]), ptr(o["summary"]),
                                               ptr(o["H"]), ptr(o["plane_inlier"]), ptr(o["plane_summary"]), ptr(o["info"]), ptr(scratch), st)
    elif what == "planar_score":
        rc = lib.affnet_epipolar_planar_score(*head, th, plane_th, rounds, seed, lo_iters, ptr(o["H"]), ptr(o["plane_inlier"]), ptr(o["plane_summary"]),
                                              ptr(o["list"]), ptr(o["n_off"]), ptr(hyp), ptr(o["counts"]), ptr(o["best"]), ptr(scratch), st)
    elif what == "plain":
        rc = lib.affnet_epipolar_verify(*head, th, rounds, seed, lo_iters, ptr(o["counts"]), ptr(o["F"]), ptr(o["inlier"]), ptr(o["summary"]), ptr(scratch), st)
    else:
        rc = lib.affnet_verify_matches(*head, plane_th, sp.HOMOGRAPHY, lo_iters, ptr(o["plane_counts"]), ptr(o["H"]), ptr(o["plane_inlier"]),
                                       ptr(o["plane_summary"]), ptr(scratch), st)
    check(rc, ctx, what)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["hyp"] = hyp.cpu().numpy()
    for k in ("summary", "plane_summary", "info", "n_off", "best"):
        out[k] = out[k].tolist()
    return out


_SCENES = {}


def scene(T, n_plane, n_off, seed):
    """Planted wall-with-things-in-front scene, computed once and shared (never modified)."""
    key = (T, n_plane, n_off, seed)
    if key not in _SCENES:
        l1, l2, tent, role, F = pp.planted_plane_scene(*key)
        _SCENES[key] = dict(l1=l1, l2=l2, tent=tent, role=role, F=F, pts=ep.gather(l1, l2, tent)[0])
    return _SCENES[key]


def same_plane(a, b, rows):
    return np.array_equal(a["H"], b["H"], equal_nan=True) and np.array_equal(a["plane_inlier"][:rows], b["plane_inlier"][:rows]) and \
        a["plane_summary"] == b["plane_summary"]


def same_result(a, b, rows, rounds):
    return np.array_equal(a["F"], b["F"], equal_nan=True) and np.array_equal(a["inlier"][:rows], b["inlier"][:rows]) and a["summary"] == b["summary"] and \
        np.array_equal(a["counts"][:rows * rounds], b["counts"][:rows * rounds])


def mirror_score(c, s, rounds, th):
    """The restatement's stages 3 to 6 behind the device's own plane."""
    T = len(c["tent"])
    return pp.score(c["l1"], c["l2"], c["tent"], th, PLANE_TH, rounds, 0, 3, plane_out=(s["H"], s["plane_inlier"][:T].astype(bool), s["plane_summary"][3]))


def check_stages(c, s, rounds, what, th=TH):
    """List, hypotheses, counts and best of a 'planar_score' result against the restatement -> (restatement, inlier matrix, Sampson gap)."""
    T = len(c["tent"])
    m = mirror_score(c, s, rounds, th)
    U, used = m["U"], m["U_used"]
    assert s["n_off"] == [U, used], (what, s["n_off"], U, used)
    assert np.array_equal(s["list"][:U], m["list"]) and (s["list"][U:] == SENT_I32).all(), what
    nh = used * rounds
    hyp, counts = s["hyp"][:nh], s["counts"][:nh]
    assert (s["hyp"][nh:] == SENT_F32).all() and (s["counts"][nh:] == SENT_I32).all(), (what, "hypotheses beyond U * rounds keep their sentinels")
    valid = np.isfinite(hyp).all(1)
    assert np.array_equal(valid, m["ok"]) and np.isnan(hyp[~valid]).all(), what
    gap = 0.0
    if valid.any():
        got, want = ep.sampson(hyp[valid].astype(np.float64), c["pts"]), ep.sampson(m["F"][valid], c["pts"])
        with np.errstate(all="ignore"):
            near = want < 10.0
            gap = float(np.abs(got - want)[near].max()) if near.any() else 0.0
        n2 = (hyp[valid].astype(np.float64) ** 2).sum(1)
        assert np.abs(n2 - 1.0).max() < 1e-6 and (np.abs(hyp[valid]).max(1) == hyp[valid].max(1)).all(), "unit norm, largest entry positive"
    assert gap <= HYP_BAR, (what, gap)
    want_counts, inl, _ = ep.score_fp32(hyp, c["pts"], th) if nh else (np.zeros(0, np.int64), np.zeros((0, T), bool), None)
    assert np.array_equal(counts, want_counts), (what, np.nonzero(counts != want_counts)[0][:8])
    b = sp.select(want_counts)
    assert s["best"] == [b, int(want_counts[b]) if b >= 0 else 0], what
    return m, inl, gap


def check_verify(c, s, m, inl, v, plain, rounds, lo_iters, what, th=TH):
    """A 'planar' result against the two contained calls' bytes and the restatement's refit from the device's own hypothesis and start mask."""
    T = len(c["tent"])
    assert same_plane(v, s, T), (what, "the full call and the stage entry find the same plane")
    assert np.array_equal(v["counts"][:T * rounds], plain["counts"][:T * rounds]), (what, "d_counts is the plain call's")
    b = s["best"][0]
    if b < 0:
        assert v["info"] == [m["U"], -1, 0, 0] and same_result(v, plain, T, rounds), what
        return None
    want = pp.refit(m["H"], c["pts"], m["off_mask"], s["hyp"][b].astype(np.float64), inl[b], th, lo_iters)
    near = want["near"]
    assert v["info"][:3] == [m["U"], b, s["best"][1]], (what, v["info"])
    n_want = int(want["mask"].sum())
    assert abs(v["info"][3] - n_want) <= int(near.sum()), (what, v["info"], n_want)
    planar = bool(v["summary"][3] & pp.FLAG_PLANAR)
    if not near.any():
        assert planar == (n_want > plain["summary"][2]), (what, n_want, plain["summary"])
    if not planar:
        assert same_result(v, plain, T, rounds), (what, "without flag 16 the outputs are affnet_epipolar_verify's bytes")
        return want
    assert v["info"][3] > plain["summary"][2] and v["summary"] == [b, s["best"][1], v["info"][3], want["flags"] | pp.FLAG_PLANAR], (what, v["summary"], v["info"])
    mask = v["inlier"][:T].astype(bool)
    assert mask.sum() == v["summary"][2] and not ((mask != want["mask"]) & ~near).any(), what
    gapr = float(np.abs(ep.sampson(v["F"], c["pts"]) - ep.sampson(want["F"], c["pts"]))[want["mask"]].max())
    assert gapr <= REFIT_BAR, (what, gapr)
    return want


@pytest.mark.parametrize("T,rounds,sc", SIZE_CASES)
def test_stages_match_the_restatement(T, rounds, sc):
    n_plane, n_off, seed, U = sc
    c = scene(T, n_plane, n_off, seed)
    s = raw(c["l1"], c["l2"], c["tent"], "planar_score", rounds=rounds)
    assert same_plane(s, raw(c["l1"], c["l2"], c["tent"], "plane"), T), "d_plane* are affnet_verify_matches' bytes"
    m, inl, gap = check_stages(c, s, rounds, (T, rounds))
    assert s["n_off"] == [U, U], ("the scene was chosen for this U", s["n_off"])
    v = raw(c["l1"], c["l2"], c["tent"], "planar", rounds=rounds)
    plain = raw(c["l1"], c["l2"], c["tent"], "plain", rounds=rounds)
    want = check_verify(c, s, m, inl, v, plain, rounds, 3, (T, rounds))
    print("T=%d rounds=%d U=%d: Sampson gap %.3g px (bar %.3g), best %s, info %s, summary %s, plain %s" % (T, rounds, U, gap, HYP_BAR, s["best"], v["info"],
                                                                                                          v["summary"], plain["summary"]))
    record_parity("plane-and-parallax hypotheses vs float64, T = %d rounds = %d U = %d" % (T, rounds, U), sampson_gap_px=gap, bar_px=HYP_BAR, best=s["best"][0],
                  best_count=s["best"][1], final=v["info"][3], plain_final=plain["summary"][2], near=int(want["near"].sum()) if want else 0)


def test_parametrised_sizes_cover_the_built_tile_edges():
    """U crosses the solve tile and the scoring tile with rounds = 1, U * rounds lands on them with rounds = 8: one below, at and one above each; U = 2 is
    the smallest input that runs the stages, T crosses the match chunk.  On the CPU the restatement leaves at most 2 % of the matches of a case in BAND."""
    from affnet_amd import _lib
    assert (_lib.EPI_TILE, _lib.EPI_CHUNK, _lib.EPI_SOLVE_TILE) == (128, 128, 64)
    assert {T for T, _, _ in SIZE_CASES} == set(SIZES) and {(T, r) for T, r, _ in SIZE_CASES} >= {(T, r) for T in SIZES for r in ROUND_CASES}
    us = {sc[3] for _, r, sc in SIZE_CASES if r == 1}
    prods = {sc[3] * r for _, r, sc in SIZE_CASES}
    for e in (_lib.EPI_TILE, _lib.EPI_SOLVE_TILE):
        assert {e - 1, e, e + 1} <= us and {e - 1, e, e + 1} <= prods
        assert any(p > 2 * e and p % e for p in prods) and any(p > 2 * e and p % e == 0 for p in prods)
    assert min(us) == 2 and {_lib.EPI_CHUNK - 1, _lib.EPI_CHUNK, _lib.EPI_CHUNK + 1} <= set(SIZES) and max(SIZES) > 2 * _lib.EPI_CHUNK
    for T, rounds, (n_plane, n_off, seed, U) in SIZE_CASES:
        c = scene(T, n_plane, n_off, seed)
        r = pp.verify_planar(c["l1"], c["l2"], c["tent"], TH, PLANE_TH, rounds, 0, 3)
        assert r["info"][0] == U and r["score"]["U_used"] == U, (T, rounds, r["info"])
        assert "refit" in r and r["refit"]["near"].sum() <= 0.02 * T, (T, rounds, int(r["refit"]["near"].sum()))


@pytest.mark.parametrize("sc,planar", pp.REFIT_SCENES)
def test_refit_is_the_kept_model(sc, planar):
    """Stage 7 seen from outside: inputs on which a refit has strictly more inliers than the best hypothesis, so that the final count, and with
    flag 16 d_model and d_inlier, are the refit's; lo_iters = 0 keeps model 0 on the same input."""
    c = scene(*sc)
    T = sc[0]
    for it in (0, 3):                      # lo_iters is the plane's too: the stages behind it are checked per value
        s = raw(c["l1"], c["l2"], c["tent"], "planar_score", rounds=1, lo_iters=it)
        m, inl, _ = check_stages(c, s, 1, (sc, it))
        b, n0 = s["best"]
        model0 = s["hyp"][b].astype(np.float64)
        v = raw(c["l1"], c["l2"], c["tent"], "planar", rounds=1, lo_iters=it)
        plain = raw(c["l1"], c["l2"], c["tent"], "plain", rounds=1, lo_iters=it)
        want = check_verify(c, s, m, inl, v, plain, 1, it, (sc, it))
        assert it == 0 or not want["near"].any(), "the scenes were chosen with no match in BAND"
        assert v["info"] == [m["U"], b, n0, int(want["mask"].sum())], (sc, it, v["info"])
        is_planar = bool(v["summary"][3] & pp.FLAG_PLANAR)
        if it == 0:
            assert want["kept"] == 0 and v["info"][3] == n0
            if is_planar:
                assert np.array_equal(v["F"], model0) and np.array_equal(v["inlier"][:T].astype(bool), inl[b]) and v["summary"] == [b, n0, n0, 16]
            continue
        if it == 3:
            assert want["kept"] > 0 and v["info"][3] > n0, (sc, "a refit must win here", want["kept"], v["info"])
            assert is_planar == planar, (sc, v["summary"], plain["summary"])
        if is_planar and want["kept"] > 0:      # d_model is a refitted model: not the hypothesis, fp64 through and through
            F = v["F"].reshape(3, 3)
            assert not np.array_equal(v["F"], model0) and np.array_equal(v["inlier"][:T].astype(bool), want["mask"])
            assert abs((F * F).sum() - 1.0) < 1e-12 and F.flat[np.argmax(np.abs(F))] > 0 and np.linalg.svd(F, compute_uv=False)[2] < 1e-12
            gap = float(np.abs(ep.sampson(v["F"], c["pts"]) - ep.sampson(want["F"], c["pts"]))[want["mask"]].max())
            print("refit %s lo_iters=%d: kept refit %d, %d -> %d inliers (plain %d), Sampson gap on the mask %.3g px (bar %.3g)" % (
                sc, it, want["kept"], n0, v["info"][3], plain["summary"][2], gap, REFIT_BAR))
            record_parity("plane-and-parallax refit vs float64, scene %s lo_iters %d" % (sc, it), sampson_gap_px=gap, bar_px=REFIT_BAR, kept=want["kept"],
                          best_count=n0, inliers=v["info"][3], plain_inliers=plain["summary"][2])


def test_refit_stops_with_flag_2():
    """The first refit's mask keeps fewer than two matches off the plane: the second iteration stops with flag 2, model 0 and its fp32 inlier set
    stay (the refit lost inliers)."""
    sc, th, rounds = pp.FEW_OFF_PLANE
    c = scene(*sc)
    T = sc[0]
    s = raw(c["l1"], c["l2"], c["tent"], "planar_score", th=th, rounds=rounds)
    m, inl, _ = check_stages(c, s, rounds, sc, th)
    b, n0 = s["best"]
    assert b >= 0 and (inl[b] & m["off_mask"]).sum() >= 2, "the first iteration refits"
    v = raw(c["l1"], c["l2"], c["tent"], "planar", th=th, rounds=rounds)
    plain = raw(c["l1"], c["l2"], c["tent"], "plain", th=th, rounds=rounds)
    want = check_verify(c, s, m, inl, v, plain, rounds, 3, sc, th)
    assert want["flags"] == 2 and want["kept"] == 0 and v["info"] == [m["U"], b, n0, n0]
    assert n0 > plain["summary"][2] and v["summary"] == [b, n0, n0, 2 | pp.FLAG_PLANAR], (v["summary"], plain["summary"])
    assert np.array_equal(v["F"], s["hyp"][b].astype(np.float64)) and np.array_equal(v["inlier"][:T].astype(bool), inl[b]), "model 0 and its mask stay"


@pytest.mark.parametrize("sc,info,summary", [((64, 40, 8, 1), [15, 13, 4, 4], [79, 5, 5, 2]), ((257, 200, 8, 4), [48, 138, 7, 7], [138, 7, 7, 16])])
def test_all_outlier_input(sc, info, summary):
    """Random matches only: the stages run (every match is "a plane" of its own), rule 8 decides.  The expected figures are the restatement's
    (tests/test_epipolar_planar_host.py): the plain bytes in the first set, flag 16 with 7 chance inliers against 6 in the second."""
    full = scene(*sc)
    t = full["tent"][full["role"] == 2]
    c = dict(full, tent=t, pts=ep.gather(full["l1"], full["l2"], t)[0])
    s = raw(c["l1"], c["l2"], t, "planar_score")
    m, inl, _ = check_stages(c, s, ROUNDS, ("outliers of", sc))
    v, plain = raw(c["l1"], c["l2"], t, "planar"), raw(c["l1"], c["l2"], t, "plain")
    want = check_verify(c, s, m, inl, v, plain, ROUNDS, 3, ("outliers of", sc))
    assert not want["near"].any() and v["info"] == info and v["summary"] == summary, (v["info"], v["summary"], plain["summary"])
    assert bool(summary[3] & pp.FLAG_PLANAR) == (not same_result(v, plain, len(t), ROUNDS))


def _descriptors(c):
    T = len(c["tent"])
    rng = np.random.default_rng(5)
    d1 = rng.normal(size=(T, 128))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 = rng.normal(size=(T, 128))                           # rows of image 2: outliers keep a random descriptor ...
    src = np.nonzero(c["role"] != 2)[0]
    d2[c["tent"][src, 1]] = d1[src] + 0.02 * rng.normal(size=(len(src), 128))      # ... planted rows a noisy copy, at the shuffled position of their frame
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    return _dev(d1, np.float32), _dev(d2, np.float32)


@pytest.mark.parametrize("sc", DEGENERATE)
def test_degenerate_scenes_end_to_end(sc):
    """Where the 8-point F is one of a family: the new call keeps the plane-and-parallax model and every planted off-plane match, the old one does not."""
    from affnet_amd import ReprojectionStuff as RS
    c = scene(*sc)
    T, off = sc[0], c["role"] == 1
    L1, L2 = _dev(c["l1"], np.float32), _dev(c["l2"], np.float32)
    t1, t2 = torch.from_numpy(c["tent"][:, 0].copy()), torch.from_numpy(c["tent"][:, 1].copy())
    F, inl, info = RS.verify_epipolar_planar(L1, L2, t1, t2, TH, PLANE_TH, ROUNDS, 0, 3)
    F0, inl0, info0 = RS.verify_epipolar(L1, L2, t1, t2, TH, ROUNDS, 0, 3)
    F1, inl1, info1 = RS.verify_matches(L1, L2, t1, t2, TH, "fundamental_planar", 3, rounds=ROUNDS, seed=0, plane_th=PLANE_TH)
    mask, mask0 = inl.cpu().numpy(), inl0.cpu().numpy()
    print("scene %s: planar %s %d inliers (%d of %d off-plane), plain %d inliers (%d of %d), n_off_plane %d, held-out median %.3g / %.3g px" % (
        sc, info["planar"], mask.sum(), mask[off].sum(), off.sum(), mask0.sum(), mask0[off].sum(), off.sum(), info["n_off_plane"],
        pp.held_out_median(F.cpu().numpy()), pp.held_out_median(F0.cpu().numpy())))
    assert info["planar"] and info["flags"] & pp.FLAG_PLANAR and mask[off].all() and info["num_inliers"] == mask.sum() > info0["num_inliers"]
    assert not info0["flags"] & pp.FLAG_PLANAR and not mask0[off].all()
    assert torch.equal(F, F1) and torch.equal(inl, inl1) and info1["planar"] and torch.equal(info["H"], info1["H"])
    assert torch.equal(info["counts"], info0["counts"]) and info["H"].shape == (3, 3) and info["plane_inliers"].dtype == torch.bool
    assert info["n_off_plane"] == int((~info["plane_inliers"]).sum().item()) and info["rounds"] == ROUNDS and info["seed"] == 0
    # the Python result is the C entry point's, and the C result is the restatement's outside BAND
    v = raw(c["l1"], c["l2"], c["tent"], "planar")
    assert np.array_equal(v["F"].reshape(3, 3), F.cpu().numpy()) and np.array_equal(v["inlier"].astype(bool), mask)
    s = raw(c["l1"], c["l2"], c["tent"], "planar_score")
    m, inl_m, gap = check_stages(c, s, ROUNDS, sc)
    want = check_verify(c, s, m, inl_m, v, raw(c["l1"], c["l2"], c["tent"], "plain"), ROUNDS, 3, sc)
    assert want is not None and want["near"].sum() <= 0.02 * T
    # the chain: guided matching under the repaired F finds at least what it finds under the plain one
    D1, D2 = _descriptors(c)
    g = RS.match_verify_guided(D1, D2, L1, L2, 0.8, TH, "fundamental_planar", rounds=ROUNDS, seed=0, plane_th=PLANE_TH)
    g0 = RS.match_verify_guided(D1, D2, L1, L2, 0.8, TH, "fundamental", rounds=ROUNDS, seed=0)
    print("guided: planar %d inliers of %d (planar %s), plain %d of %d" % (g[3].sum(), g[0].numel(), g[4]["planar"], g0[3].sum(), g0[0].numel()))
    assert int(g[3].sum()) >= int(g0[3].sum()) and g[4]["num_inliers"] == int(g[3].sum()) and {"planar", "H", "plane_inliers", "n_off_plane", "seed_stage"} <= set(g[4])
    a = RS.match_and_verify(D1, D2, L1, L2, 0.8, TH, "fundamental_planar", 3, rounds=ROUNDS, seed=0, plane_th=PLANE_TH)
    m1, m2, _, _ = RS.match_snn(D1, D2, 0.8)
    Fa, inla, infoa = RS.verify_epipolar_planar(L1, L2, m1, m2, TH, PLANE_TH, ROUNDS, 0, 3)
    assert torch.equal(a[0], m1) and torch.equal(a[2], Fa) and torch.equal(a[3], inla) and a[4]["planar"] == infoa["planar"] and a[4]["n_off_plane"] == infoa["n_off_plane"]
    record_parity("plane-aware epipolar verification, degenerate scene %s" % (sc,), inliers=int(mask.sum()), plain_inliers=int(mask0.sum()), off_plane=int(off.sum()),
                  off_plane_found=int(mask[off].sum()), plain_off_plane_found=int(mask0[off].sum()), guided_inliers=int(g[3].sum()), guided_plain_inliers=int(g0[3].sum()))


def test_determinism_and_stale_workspace():
    c = scene(*DEGENERATE[0])
    runs = [raw(c["l1"], c["l2"], c["tent"], "planar"), raw(c["l1"], c["l2"], c["tent"], "planar"), raw(c["l1"], c["l2"], c["tent"], "planar", scratch_fill=0xFF)]
    runs_s = [raw(c["l1"], c["l2"], c["tent"], "planar_score"), raw(c["l1"], c["l2"], c["tent"], "planar_score", scratch_fill=0xFF)]
    for group in (runs, runs_s):
        for x in group[1:]:
            for k, v in group[0].items():
                assert np.array_equal(v, x[k], equal_nan=True) if isinstance(v, np.ndarray) else v == x[k], k
    assert runs[0]["summary"][3] & pp.FLAG_PLANAR
    o = raw(c["l1"], c["l2"], c["tent"], "planar_score", seed=1)
    assert not np.array_equal(o["hyp"], runs_s[0]["hyp"], equal_nan=True) and o["n_off"] == runs_s[0]["n_off"]


def test_count_pointer_limits_what_is_read_and_written():
    sc = (257,) + SCENE_OF[257][:3]
    c = scene(*sc)
    ref, ref_s = raw(c["l1"], c["l2"], c["tent"], "planar"), raw(c["l1"], c["l2"], c["tent"], "planar_score")
    # capacity 512, 257 valid rows; the rows behind the count point (with valid indices) at frames that are all NaN
    n = c["l1"].shape[0]
    l1 = np.concatenate([c["l1"], np.full((4, 2, 3), np.nan, np.float32)])
    l2 = np.concatenate([c["l2"], np.full((4, 2, 3), np.nan, np.float32)])
    tent = np.concatenate([c["tent"], np.stack([n + np.arange(255) % 4, n + np.arange(255) % 4], 1).astype(np.int32)])
    r = raw(l1, l2, tent, "planar", count=257, cap=512)
    nh = 257 * ROUNDS
    assert same_result(r, ref, 257, ROUNDS) and same_plane(r, ref, 257) and r["info"] == ref["info"]
    assert (r["counts"][nh:] == SENT_I32).all() and (r["inlier"][257:] == SENT_U8).all() and (r["plane_inlier"][257:] == SENT_U8).all()
    s = raw(l1, l2, tent, "planar_score", count=257, cap=512)
    U = ref_s["n_off"][0]
    assert s["n_off"] == ref_s["n_off"] and s["best"] == ref_s["best"] and np.array_equal(s["list"][:U], ref_s["list"][:U]) and (s["list"][U:] == SENT_I32).all()
    assert np.array_equal(s["hyp"][:U * ROUNDS], ref_s["hyp"][:U * ROUNDS]) and (s["hyp"][U * ROUNDS:] == SENT_F32).all()
    assert np.array_equal(s["counts"][:U * ROUNDS], ref_s["counts"][:U * ROUNDS]) and (s["counts"][U * ROUNDS:] == SENT_I32).all()
    # a count above the capacity is clamped; a count of zero and a capacity of zero give the plain empty result
    over = raw(c["l1"], c["l2"], c["tent"], "planar", count=100000, cap=257)
    assert same_result(over, ref, 257, ROUNDS) and over["info"] == ref["info"]
    zero = raw(l1, l2, tent, "planar", count=0, cap=512)
    assert zero["summary"] == [-1, 0, 0, 1] and zero["plane_summary"] == [-1, 0, 0, 1] and zero["info"] == [0, -1, 0, 0] and not zero["F"].any()
    assert (zero["counts"] == SENT_I32).all() and (zero["inlier"] == SENT_U8).all() and (zero["plane_inlier"] == SENT_U8).all()
    empty = raw(c["l1"], c["l2"], np.zeros((0, 2), np.int32), "planar")
    assert empty["summary"] == [-1, 0, 0, 1] and empty["info"] == [0, -1, 0, 0] and not empty["F"].any()


def test_inputs_without_parallax_give_the_plain_bytes():
    c = scene(64, 40, 8, 1)
    role, tent = c["role"], c["tent"]
    on = np.flatnonzero(role == 0)
    # three neighbouring rows of the plane are what one affine hypothesis explains: U = 0 around plane row 0, U = 1 around plane row 1
    cases = {"T=2": tent[:2], "T=3": tent[:3], "T=3, U=0": tent[pp.neighbours(c["l1"], on, 0)], "T=3, U=1": tent[pp.neighbours(c["l1"], on, 1)], "pure plane": tent[on], "U=1": tent[np.sort(np.append(on, np.flatnonzero(role == 1)[0]))]}
    for name, t in cases.items():
        v, plain, plane = raw(c["l1"], c["l2"], t, "planar"), raw(c["l1"], c["l2"], t, "plain"), raw(c["l1"], c["l2"], t, "plane")
        want = pp.verify_planar(c["l1"], c["l2"], t, TH, PLANE_TH, ROUNDS, 0, 3)
        print(name, v["info"], v["summary"], v["plane_summary"], want["info"])
        assert same_result(v, plain, len(t), ROUNDS) and same_plane(v, plane, len(t)), name
        if name != "T=3" or want["info"][1] < 0:
            assert v["info"] == want["info"] and v["info"][1:] == [-1, 0, 0], (name, v["info"], want["info"])
    # invalid rows are not on the list: out-of-range indices (never loaded through), a centre that is not finite
    a, t2 = c["l1"].copy(), tent.copy()
    a[tent[5, 0], 0, 2] = np.inf
    t2[6], t2[7], t2[8] = (-1, 0), (0, len(c["l2"])), (2 ** 31 - 1, -2 ** 31)
    s = raw(a, c["l2"], t2, "planar_score")
    bad = dict(c, l1=a, tent=t2, pts=ep.gather(a, c["l2"], t2)[0])
    m, inl, _ = check_stages(bad, s, ROUNDS, "bad rows")
    assert not np.isin([5, 6, 7, 8], s["list"][:s["n_off"][0]]).any() and not inl[:, [5, 6, 7, 8]].any()
    # frames of zero size: no hypothesis of either kind, the plane summary has flag 1, the stages are skipped whatever U is
    z1, z2 = c["l1"].copy(), c["l2"].copy()
    z1[:, :, :2] = 0.0
    z2[:, :, :2] = 0.0
    v = raw(z1, z2, tent, "planar")
    assert v["plane_summary"] == [-1, 0, 0, 1] and v["info"] == [64, -1, 0, 0] and v["summary"] == [-1, 0, 0, 1] and same_result(v, raw(z1, z2, tent, "plain"), 64, ROUNDS)
