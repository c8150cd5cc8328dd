"""CPU: the restatement of the epipolar-verification rules (tests/_epipolar_fp64.py) does what it is for on planted scenes with depth and on
planted planar scenes, the hash gives usable triplets, BAND is what the file says it is, and the new entry points are part of the boundary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _epipolar_fp64 as ep
import _spatial_fp64 as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, ROUNDS = 2.0, 8


@pytest.fixture(scope="module")
def runs():
    """(scene) -> (ground-truth mask, result of the whole restatement); computed once, never modified."""
    out = {}
    for T, share, seed in ep.SCENES:
        l1, l2, tent, _, F = ep.planted_two_view(T, share, seed)
        r = ep.verify(l1, l2, tent, TH, ROUNDS, 0, 3)
        out[(T, share, seed)] = (ep.sampson(F.reshape(9), r["hyp"]["pts"]) <= TH, r)
    for T, seed in ep.PLANAR:
        l1, l2, tent, pl = sp.planted(T, seed)
        out[(T, seed)] = (pl, ep.verify(l1, l2, tent, TH, ROUNDS, 0, 3))
    return out


def test_header_declares_and_lib_binds_the_entry_points():
    from affnet_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "affnet_hip.h")).read(), flags=re.S)
    for name, nargs in (("affnet_epipolar_scratch_bytes", 2), ("affnet_epipolar_score", 16), ("affnet_epipolar_verify", 18)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    for name, val in (("MAX_ROUNDS", _lib.EPI_MAX_ROUNDS), ("TILE", _lib.EPI_TILE), ("CHUNK", _lib.EPI_CHUNK), ("SOLVE_TILE", _lib.EPI_SOLVE_TILE)):
        assert re.search(r"#define\s+AFFNET_EPI_%s\s+%d\b" % (name, val), hdr), name
    assert _lib.EPI_MAX_ROUNDS == ep.MAX_ROUNDS == 64


def test_scratch_bytes_are_monotone():
    from affnet_amd import _lib
    f = _lib.lib.affnet_epipolar_scratch_bytes
    ts = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 2000, 100000)
    for r in (1, 8, 64):
        sizes = [f(t, r) for t in ts]
        assert sizes[1] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] >= 100000 * (65 + 36 * r), "four float4 and one mask byte per row, nine floats per hypothesis"
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
        ok = dict(l1=p, n1=4, l2=p, n2=4, tent=p, count=None, t=4, th=2.0, rounds=8, seed=0, it=3, hyp=p, counts=p, best=p, F=p, inl=p, summ=p, scr=p)

        def verify(**kw):
            a = dict(ok, **kw)
            return lib.affnet_epipolar_verify(h, a["l1"], a["n1"], a["l2"], a["n2"], a["tent"], a["count"], a["t"], a["th"], a["rounds"], a["seed"], a["it"],
                                              a["counts"], a["F"], a["inl"], a["summ"], a["scr"], None)

        def score(**kw):
            a = dict(ok, **kw)
            return lib.affnet_epipolar_score(h, a["l1"], a["n1"], a["l2"], a["n2"], a["tent"], a["count"], a["t"], a["th"], a["rounds"], a["seed"], a["hyp"],
                                             a["counts"], a["best"], a["scr"], None)
        common = [dict(l1=None), dict(l2=None), dict(tent=None), dict(counts=None), dict(scr=None), dict(t=-1), dict(n1=-1), dict(n2=-1), dict(th=0.0),
                  dict(th=-1.0), dict(th=float("nan")), dict(th=float("inf")), dict(rounds=0), dict(rounds=-1), dict(rounds=65), dict(scr=C.c_void_p(4100)),
                  dict(t=2 ** 31 - 1, rounds=2), dict(t=2 ** 26, rounds=32)]
        for kw in common + [dict(F=None), dict(inl=None), dict(summ=None), dict(it=-1), dict(it=9)]:
            assert verify(**kw) == _lib.ERR_INVALID, kw
            assert b"epipolar_verify" in lib.affnet_last_error(h), kw
        for kw in common + [dict(best=None)]:
            assert score(**kw) == _lib.ERR_INVALID, kw
            assert b"epipolar_score" in lib.affnet_last_error(h), kw
    finally:
        lib.affnet_ctx_destroy(h)


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import ReprojectionStuff as RS
    for name in ("verify_epipolar", "enqueue_verify_epipolar", "sampson_distance"):
        assert getattr(affnet_amd, name) is getattr(RS, name)
    with pytest.raises(RuntimeError):
        RS.verify_epipolar(np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), [0], [0])        # no CPU path
    with pytest.raises(RuntimeError):
        RS.verify_matches(np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), [0], [0], model="fundamental")


def test_lowbias32_known_values():
    """The finaliser as published (Wellons, "Prospecting for hash functions"): 0 is its fixed point, and it is a bijection of uint32 - no two of a
    run of inputs collide."""
    assert int(ep.lowbias32(0)) == 0
    x = 1
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    assert int(ep.lowbias32(1)) == x
    v = ep.lowbias32(np.arange(1 << 16))
    assert len(np.unique(v)) == 1 << 16 and v.max() < 1 << 32


@pytest.mark.parametrize("T", [3, 4, 5, 64, 1000])
def test_hash_gives_distinct_triplets_in_range(T):
    for rounds, seed in ((1, 0), (8, 0), (8, 12345), (64, 0xFFFFFFFF)):
        m = ep.members(T, rounds, seed)
        assert m.shape == (T * rounds, 3) and m.min() >= 0 and m.max() < T
        assert (m[:, 0] == np.repeat(np.arange(T), rounds)).all()
        assert (m[:, 0] != m[:, 1]).all() and (m[:, 0] != m[:, 2]).all() and (m[:, 1] != m[:, 2]).all()
    if T >= 64:         # the partners are spread: a seed's rounds do not repeat one triplet, another seed gives other triplets
        m = ep.members(T, 8, 0)
        assert len(np.unique(m, axis=0)) > 0.95 * len(m)
        assert (ep.members(T, 8, 1) != m).any(1).mean() > 0.9


@pytest.mark.parametrize("scene", ep.SCENES)
def test_restatement_recovers_a_scene_with_depth(runs, scene):
    gt, r = runs[scene]
    assert r["summary"][0] >= 0 and r["summary"][3] == 0
    kept, others = int((r["mask"] & gt).sum()), int((r["mask"] & ~gt).sum())
    print("scene %s: best %d with %d, kept %d of %d, others %d" % (scene, r["summary"][0], r["summary"][1], kept, gt.sum(), others))
    assert kept >= 0.95 * gt.sum(), (kept, gt.sum())
    assert others <= 0.05 * gt.sum(), (others, gt.sum())
    F = r["F"].reshape(3, 3)
    assert abs(np.sqrt((F * F).sum()) - 1.0) < 1e-12 and F.flat[np.argmax(np.abs(F))] > 0
    assert np.linalg.svd(F, compute_uv=False)[2] < 1e-9, "a refitted model has rank 2"


@pytest.mark.parametrize("scene", ep.PLANAR)
def test_restatement_keeps_the_planted_rows_of_a_planar_scene(runs, scene):
    """F is degenerate on a plane (one of a family), the inlier test is not: the planted rows stay."""
    pl, r = runs[scene]
    kept = int((r["mask"] & pl).sum())
    print("planar %s: kept %d of %d, mask %d" % (scene, kept, pl.sum(), r["mask"].sum()))
    assert r["summary"][0] >= 0 and kept >= 0.95 * pl.sum(), (kept, pl.sum())


def test_band_is_ten_times_the_fp32_spread(runs):
    worst = 0.0
    for gt, r in runs.values():
        e64 = ep.sampson(r["hyp"]["hyp32"].astype(np.float64), r["hyp"]["pts"])
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.abs(r["e32"] - e64)[e64 < 10.0].max()))
    print("largest fp32-vs-fp64 difference of sqrt(e) below 10 px: %.4g px, BAND %.3g" % (worst, ep.BAND))
    assert 10 * worst <= ep.BAND <= 10.2 * worst


def test_restatement_edge_rules():
    l1, l2, tent, _, _ = ep.planted_two_view(64, 0.5, 3)
    # T < 3: nothing valid
    for T in (0, 1, 2):
        r = ep.verify(l1, l2, tent[:T], TH, ROUNDS, 0, 3)
        assert r["summary"] == [-1, 0, 0, 1] and not r["hyp"]["ok"].any() and len(r["counts"]) == T * ROUNDS
    # lo_iters = 0: model 0 is the stored fp32 hypothesis, its mask the fp32 inlier set
    r = ep.verify(l1, l2, tent, TH, ROUNDS, 0, 0)
    b = r["best"]
    assert np.array_equal(r["F"], r["hyp"]["hyp32"][b].astype(np.float64)) and r["summary"] == [b, r["counts"][b], r["counts"][b], 0]
    # invalid rows: NaN in a shape (member unusable, centres usable), infinite centre, out-of-range indices
    a, bb, t2 = l1.copy(), l2.copy(), tent.copy()
    bb[tent[4, 1], 0, 1] = np.nan
    a[tent[5, 0], 0, 2] = np.inf
    t2[6] = (-1, 0)
    t2[7] = (0, len(bb))
    hy = ep.hypotheses(a, bb, t2, ROUNDS, 0)
    assert hy["match_ok"][4] and not hy["member_ok"][4] and not hy["match_ok"][[5, 6, 7]].any()
    bad = np.isin(hy["mem"], [4, 5, 6, 7]).any(1)
    assert bad.any() and not hy["ok"][bad].any() and hy["ok"][~bad].all() and np.isnan(hy["F"][bad]).all()
    counts, inl, _ = ep.score_fp32(hy["hyp32"], hy["pts"], TH)
    assert (counts[bad] == 0).all() and not inl[:, [5, 6, 7]].any()
    # a singular frame among the members: a frame of zero size in both images is three coincident correspondences, equal rows of the system
    z1, z2 = l1.copy(), l2.copy()
    z1[tent[9, 0], :, :2] = 0.0
    z2[tent[9, 1], :, :2] = 0.0
    hz = ep.hypotheses(z1, z2, tent, ROUNDS, 0)
    with9 = (hz["mem"] == 9).any(1)
    assert with9.sum() >= ROUNDS and not hz["ok"][with9].any() and hz["ok"][~with9].all()
    # five consistent rows: flag 2; collinear centres: flag 4
    r = ep.verify(*ep.few_rows(), TH, ROUNDS, 0, 3)
    assert r["summary"][3] == 2 and 3 <= r["summary"][2] == r["summary"][1] <= 5, r["summary"]
    r = ep.verify(*ep.collinear_rows(), TH, ROUNDS, 0, 3)
    assert r["summary"][3] == 4 and r["summary"][2] == r["summary"][1] >= 8, r["summary"]
