"""CPU: the restatement of the plane-aware epipolar verification rules (tests/_epipolar_planar_fp64.py) does what it is for on planted
wall-with-things-in-front scenes, the degenerate inputs give the plain result, and the new entry points are part of the boundary.

MEASURED on the CPU with the restatement as committed (inl_th 2 px, plane_th 3 px, rounds 8, seed 0, lo_iters 3; held-out = median Sampson
distance of 400 noise-free correspondences at depths 3..10 under the returned F):

  T / on plane / off plane / seed | plain: off-plane found, held-out median | planar result: off-plane found, held-out median, flag 16
  200 / 120 / 16 / 5              |  2 of 16, 16.78 px                      | 16 of 16, 0.34 px, yes
  128 /  90 /  6 / 6              |  2 of  6, 13.34 px                      |  6 of  6, 0.36 px, yes
  129 /  80 / 12 / 2              |  3 of 12, 15.63 px                      | 12 of 12, 0.32 px, yes
   64 /  40 /  8 / 1              |  0 of  8, 33.92 px                      |  8 of  8, 0.68 px, yes
  257 / 160 / 24 / 3              | 24 of 24,  0.05 px                      | 24 of 24, 0.05 px, no (a tie at 186 inliers: the plain model stays)
  257 / 200 /  8 / 4              |  3 of  8, 17.36 px                      |  8 of  8, 0.22 px, yes"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _epipolar_fp64 as ep
import _epipolar_planar_fp64 as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, PLANE_TH, ROUNDS = 2.0, 3.0, 8
NAMES = (("affnet_epipolar_planar_scratch_bytes", 2), ("affnet_epipolar_planar_score", 23), ("affnet_epipolar_verify_planar", 23))


@pytest.fixture(scope="module")
def runs():
    """scene -> (role, result of the whole restatement); computed once, never modified."""
    out = {}
    for sc in pp.SCENES:
        l1, l2, tent, role, _ = pp.planted_plane_scene(*sc)
        out[sc] = (role, pp.verify_planar(l1, l2, tent, TH, PLANE_TH, ROUNDS, 0, 3))
    return out


def test_header_declares_and_lib_binds_the_entry_points():
    from affnet_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "affnet_hip.h")).read(), flags=re.S)
    for name, nargs in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define\s+AFFNET_EPI_FLAG_PLANAR\s+%d\b" % _lib.EPI_FLAG_PLANAR, hdr) and _lib.EPI_FLAG_PLANAR == pp.FLAG_PLANAR == 16


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import ReprojectionStuff as RS
    for name in ("verify_epipolar_planar", "enqueue_verify_epipolar_planar"):
        assert getattr(affnet_amd, name) is getattr(RS, name)
    with pytest.raises(RuntimeError):
        RS.verify_epipolar_planar(np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), [0], [0])        # no CPU path
    with pytest.raises(RuntimeError):
        RS.verify_matches(np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), [0], [0], model="fundamental_planar")


def test_scratch_bytes_are_monotone_and_aligned():
    from affnet_amd import _lib
    f = _lib.lib.affnet_epipolar_planar_scratch_bytes
    ts = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 2000, 100000)
    for r in (1, 8, 64):
        sizes = [f(t, r) for t in ts]
        assert sizes[1] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes), sizes
        assert all(f(t, r) >= _lib.lib.affnet_epipolar_scratch_bytes(t, r) + t * (16 + 8 + 3 + 40 * r) for t in ts), "the two calls' scratch and this one's own lists"
    for t in ts:
        sizes = [f(t, r) for r in range(1, 65)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), t
    assert f(-5, 8) == f(0, 8) and f(100, -1) == f(100, 0)


def test_bad_arguments_are_refused_before_any_device_work():
    """The argument checks run on the host, in front of the first launch: they need no GPU."""
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        p = C.c_void_p(4096)            # never dereferenced: every call below is refused
        ok = dict(l1=p, n1=4, l2=p, n2=4, tent=p, count=None, t=4, th=2.0, pth=3.0, rounds=8, seed=0, it=3, hyp=p, counts=p, best=p, F=p, inl=p, summ=p, H=p,
                  pinl=p, psumm=p, info=p, lst=p, noff=p, scr=p)

        def verify(**kw):
            a = dict(ok, **kw)
            return lib.affnet_epipolar_verify_planar(h, a["l1"], a["n1"], a["l2"], a["n2"], a["tent"], a["count"], a["t"], a["th"], a["pth"], a["rounds"], a["seed"],
                                                     a["it"], a["counts"], a["F"], a["inl"], a["summ"], a["H"], a["pinl"], a["psumm"], a["info"], a["scr"], None)

        def score(**kw):
            a = dict(ok, **kw)
            return lib.affnet_epipolar_planar_score(h, a["l1"], a["n1"], a["l2"], a["n2"], a["tent"], a["count"], a["t"], a["th"], a["pth"], a["rounds"], a["seed"],
                                                    a["it"], a["H"], a["pinl"], a["psumm"], a["lst"], a["noff"], a["hyp"], a["counts"], a["best"], a["scr"], None)
        common = [dict(l1=None), dict(l2=None), dict(tent=None), dict(counts=None), dict(scr=None), dict(t=-1), dict(n1=-1), dict(n2=-1), dict(th=0.0),
                  dict(th=-1.0), dict(th=float("nan")), dict(th=float("inf")), dict(rounds=0), dict(rounds=-1), dict(rounds=65), dict(scr=C.c_void_p(4100)),
                  dict(t=2 ** 31 - 1, rounds=2), dict(t=2 ** 26, rounds=32), dict(it=-1), dict(it=9), dict(pth=0.0), dict(pth=-3.0), dict(pth=float("nan")),
                  dict(pth=float("inf")), dict(H=None), dict(pinl=None), dict(psumm=None)]
        for kw in common + [dict(F=None), dict(inl=None), dict(summ=None), dict(info=None)]:
            assert verify(**kw) == _lib.ERR_INVALID, kw
            assert b"epipolar_verify_planar" in lib.affnet_last_error(h), kw
        for kw in common + [dict(best=None), dict(lst=None), dict(noff=None)]:
            assert score(**kw) == _lib.ERR_INVALID, kw
            assert b"epipolar_planar_score" in lib.affnet_last_error(h), kw
    finally:
        lib.affnet_ctx_destroy(h)


def test_partners_are_distinct_and_in_range():
    for U in (2, 3, 63, 64, 65, 1000):
        for rounds, seed in ((1, 0), (8, 0), (64, 0xFFFFFFFF)):
            a, b = pp.partners(U, rounds, seed)
            assert (a == np.repeat(np.arange(U), rounds)).all() and b.min() >= 0 and b.max() < U and (a != b).all()
    a, b = pp.partners(1000, 8, 0)
    assert np.array_equal(b, ep.members(1000, 8, 0)[:, 1]), "the partner is member 1 of the 8-point hash over U instead of T"


def test_lines_pass_through_the_epipole():
    """Noise-free correspondences off the plane, the planted H: every parallax line contains the planted epipole of image 2, K t."""
    pts = pp.held_out()
    l, ok = pp.lines(pp.plane_H(), pts)
    e = ep.K @ ep.TRANS
    e = e / e[2]
    assert ok.all() and np.abs(l @ e).max() < 1e-6, "distance of the epipole from each line, px"
    F, fin = pp.model(e[None], pp.plane_H())
    assert fin[0] and np.nanmax(ep.sampson(F[0], pts)) < 1e-6
    G = ep.planted_F().reshape(9)
    assert np.abs(np.abs(F[0] @ G) - 1.0) < 1e-9, "[e]x H is the planted F up to sign"


def test_degenerate_scenes_are_repaired(runs):
    """Where the plain model finds fewer than half of the planted off-plane matches, the plane-and-parallax model is kept and contains all of them."""
    qualify = 0
    for sc, (role, r) in runs.items():
        off = role == 1
        plain_found, found = int(r["plain"]["mask"][off].sum()), int(r["mask"][off].sum())
        print("scene %s: plain %d of %d off-plane, %d inliers, held-out median %.3g px; result %d of %d, %d inliers, %.3g px, flags %d, info %s" % (
            sc, plain_found, off.sum(), r["plain"]["summary"][2], pp.held_out_median(r["plain"]["F"]), found, off.sum(), r["summary"][2],
            pp.held_out_median(r["F"]), r["summary"][3], r["info"]))
        if 2 * plain_found < off.sum():
            qualify += 1
            assert r["planar"] and r["summary"][3] & pp.FLAG_PLANAR and found == off.sum(), sc
            assert pp.held_out_median(r["F"]) < 1.0 < pp.held_out_median(r["plain"]["F"]), sc
    assert qualify >= 2, "the scenes no longer show the degeneracy"
    assert 2 * int(runs[(200, 120, 16, 5)][1]["plain"]["mask"][runs[(200, 120, 16, 5)][0] == 1].sum()) < 16
    assert 2 * int(runs[(128, 90, 6, 6)][1]["plain"]["mask"][runs[(128, 90, 6, 6)][0] == 1].sum()) < 6


@pytest.mark.parametrize("scene", pp.SCENES)
def test_result_has_at_least_the_plain_inliers(runs, scene):
    role, r = runs[scene]
    plain = r["plain"]
    assert r["summary"][2] == int(r["mask"].sum()) >= plain["summary"][2]
    assert r["info"][0] == len(r["score"]["list"]) and r["info"][3] >= r["info"][2] > 0
    if r["planar"]:
        assert r["summary"][2] > plain["summary"][2] and r["summary"][:3] == r["info"][1:]
        F = r["F"].reshape(3, 3)
        # model 0 (a float32 hypothesis widened) may be the kept one: unit norm and rank 2 to float32 rounding
        assert abs(np.sqrt((F * F).sum()) - 1.0) < 1e-6 and F.flat[np.argmax(np.abs(F))] > 0
        assert np.linalg.svd(F, compute_uv=False)[2] < 1e-6, "[e]x H has rank 2"
    else:
        assert r["summary"] == plain["summary"] and np.array_equal(r["F"], plain["F"]) and np.array_equal(r["mask"], plain["mask"])
    # the off-plane list: ascending, usable, outside the plane mask; the plane holds the planted plane rows
    lst = r["score"]["list"]
    assert (np.diff(lst) > 0).all() and not r["plane"]["mask"][lst].any()
    assert r["plane"]["mask"][role == 0].mean() > 0.95


@pytest.mark.parametrize("sc,planar", pp.REFIT_SCENES)
def test_refit_scenes_are_won_by_a_refit(sc, planar):
    """What the GPU tests of the refit rest on: on these inputs a refitted epipole has strictly more inliers than the best hypothesis."""
    l1, l2, tent, _, _ = pp.planted_plane_scene(*sc)
    r = pp.verify_planar(l1, l2, tent, TH, PLANE_TH, 1, 0, 3)
    rf = r["refit"]
    assert rf["kept"] > 0 and rf["flags"] == 0 and r["info"][3] > r["info"][2] and not rf["near"].any() and r["planar"] == planar, (r["info"], r["plain"]["summary"])
    assert r["planar"] or r["info"][3] == r["plain"]["summary"][2], "where the plain model stays it is by a tie"
    F = rf["F"].reshape(3, 3)
    assert abs(np.sqrt((F * F).sum()) - 1.0) < 1e-12 and np.linalg.svd(F, compute_uv=False)[2] < 1e-12
    r0 = pp.verify_planar(l1, l2, tent, TH, PLANE_TH, 1, 0, 0)
    assert r0["refit"]["kept"] == 0 and r0["info"][3] == r0["info"][2]


def test_refit_stops_with_flag_2_below_two_off_plane_inliers():
    sc, th, rounds = pp.FEW_OFF_PLANE
    l1, l2, tent, _, _ = pp.planted_plane_scene(*sc)
    r = pp.verify_planar(l1, l2, tent, th, PLANE_TH, rounds, 0, 3)
    b = r["score"]["best"]
    assert (r["score"]["inl"][b] & r["score"]["off_mask"]).sum() >= 2, "the first iteration refits; its mask is what stops the second"
    assert r["refit"]["flags"] == 2 and r["refit"]["kept"] == 0 and pp.refit(r["score"]["H"], r["score"]["pts"], r["score"]["off_mask"],
                                                                             r["F"], r["score"]["inl"][b], th, 1)["flags"] == 0
    assert r["planar"] and r["summary"] == [b, r["info"][2], r["info"][2], 2 | pp.FLAG_PLANAR]
    assert np.array_equal(r["F"], r["score"]["hyp32"][b].astype(np.float64)) and np.array_equal(r["mask"], r["score"]["inl"][b])
    # a rank-1 N (every line of S the same) is flag 4: the restatement's fit refuses it
    pts = r["score"]["pts"]
    lst = r["score"]["list"]
    assert pp.fit(r["score"]["H"], pts[[lst[0], lst[0]]], np.ones(2, bool)) is None


def _same_as_plain(r):
    p = r["plain"]
    return (not r["planar"] and r["info"][1:] == [-1, 0, 0] and r["summary"] == p["summary"] and np.array_equal(r["F"], p["F"], equal_nan=True)
            and np.array_equal(r["mask"], p["mask"]))


def test_inputs_without_parallax_give_the_plain_result():
    l1, l2, tent, role, _ = pp.planted_plane_scene(64, 40, 8, 1)
    on = np.flatnonzero(role == 0)
    # Three neighbouring rows of the plane (below four rows there is no homography refit: the plane is what one affine hypothesis explains
    # within plane_th, its neighbours): U = 0 around plane row 0, U = 1 around plane row 1
    for T in (0, 2, 3):
        for k, U in ((0, 0), (1, 1)):
            r = pp.verify_planar(l1, l2, tent[pp.neighbours(l1, on, k)[:T]], TH, PLANE_TH, ROUNDS, 0, 3)
            assert (T < 3 or r["info"][0] == U) and r["info"][0] < 2 and _same_as_plain(r), (T, k, r["info"])
    # Three rows of which one is "the plane" (the first hypothesis counts itself): U = 2, by rule 3 the stages run - two lines and one model,
    # three inliers against the plain model's three: the tie keeps the plain bytes
    r = pp.verify_planar(l1, l2, tent[:3], TH, PLANE_TH, ROUNDS, 0, 3)
    assert r["info"][0] == 2 and not r["planar"] and r["summary"] == r["plain"]["summary"] and np.array_equal(r["F"], r["plain"]["F"])
    # U = 0: the plane rows alone; U = 1: one more row
    r = pp.verify_planar(l1, l2, tent[on], TH, PLANE_TH, ROUNDS, 0, 3)
    assert r["info"][0] == 0 and _same_as_plain(r), "a pure plane"
    r1 = pp.verify_planar(l1, l2, tent[np.sort(np.append(on, np.flatnonzero(role == 1)[0]))], TH, PLANE_TH, ROUNDS, 0, 3)
    assert r1["info"][0] == 1 and _same_as_plain(r1)
    # all outliers.  Random frames: every match is a valid affine hypothesis that counts itself, so the plane stage finds "a plane" and the
    # stages run (two lines meet in a point: every hypothesis has its two members as inliers); the decision rule alone keeps the result sound.
    # Three fixed outlier sets, with what the restatement gives for them: a tie and a loss keep the plain bytes, and in the third the
    # plane-and-parallax model has 7 chance inliers against 6 and is returned with flag 16 - an all-outlier input is not a special case.
    out = np.flatnonzero(role == 2)
    for sc, info, summary, plain in (((64, 40, 8, 1), [15, 13, 4, 4], [79, 5, 5, 2], [79, 5, 5, 2]),
                                     ((200, 120, 16, 5), [63, 3, 6, 6], [100, 6, 6, 2], [100, 6, 6, 2]),
                                     ((257, 200, 8, 4), [48, 138, 7, 7], [138, 7, 7, 16], [388, 6, 6, 2])):
        a, b, t, r4, _ = pp.planted_plane_scene(*sc)
        ro = pp.verify_planar(a, b, t[r4 == 2], TH, PLANE_TH, ROUNDS, 0, 3)
        assert ro["info"] == info and ro["summary"] == summary and ro["plain"]["summary"] == plain, (sc, ro["info"], ro["summary"], ro["plain"]["summary"])
        if summary[3] & pp.FLAG_PLANAR:
            assert ro["planar"] and ro["mask"].sum() == 7 and not np.array_equal(ro["F"], ro["plain"]["F"])
        else:
            assert np.array_equal(ro["F"], ro["plain"]["F"]) and np.array_equal(ro["mask"], ro["plain"]["mask"])
    # Frames of zero size: no match is a hypothesis of either kind, the plane summary has flag 1, the stages are skipped
    z1, z2 = l1.copy(), l2.copy()
    z1[:, :, :2] = 0.0
    z2[:, :, :2] = 0.0
    rz = pp.verify_planar(z1, z2, tent[out], TH, PLANE_TH, ROUNDS, 0, 3)
    assert rz["plane"]["summary"] == [-1, 0, 0, 1] and rz["info"][0] == len(out) and rz["summary"] == [-1, 0, 0, 1] and _same_as_plain(rz)
    # a plane summary with flag 1 skips the stages whatever U is
    lst, used = pp.off_plane(np.ones(5, bool), np.zeros(5, bool), 1)
    assert len(lst) == 5 and used == 0 and pp.off_plane(np.ones(5, bool), np.zeros(5, bool), 0)[1] == 5
