"""CPU: the float64 restatement of the spatial-verification rules (tests/_spatial_fp64.py) does what it is for on the planted inputs, the
preconditions the GPU tests of csrc/spatial.hip rely on hold for the chosen cases, and the new entry points are part of the boundary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _spatial_fp64 as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = 3.0
# (T, seed): T = 1000 runs on one seed to keep the suite quick; every case here meets both preconditions below for both models
CASES = [(65, 0), (65, 1), (65, 2), (65, 3), (257, 0), (257, 1), (257, 2), (257, 3), (1000, 0)]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for T, seed in CASES:
        l1, l2, tent, pl = sp.planted(T, seed)
        sc = sp.score(l1, l2, tent, TH)
        c32, inl32, e32 = sp.score_fp32(l1, l2, tent, TH)
        out[(T, seed)] = dict(l1=l1, l2=l2, tent=tent, planted=pl, sc=sc, c32=c32, inl32=inl32, e32=e32)
    return out


@pytest.mark.parametrize("case", CASES)
def test_restatement_recovers_the_planted_set_and_model(cases, case):
    c = cases[case]
    r = sp.verify(c["l1"], c["l2"], c["tent"], TH, sp.HOMOGRAPHY, 3)
    assert r["best"] >= 0 and c["planted"][r["best"]], "the best hypothesis is a planted match"
    assert r["summary"][3] == 0
    assert np.array_equal(r["mask"], c["planted"]), "three homography refits return exactly the planted inlier set"
    # "to within the noise".  The kept model is the EARLIEST one with the largest mask (rule 6), possibly fitted to a handful of pairs: what it
    # guarantees is the mask itself, every planted pair within th of its noisy position.  The fit the rules prescribe, on the whole planted set, is
    # closer to the noise-free positions than the 0.3 px (per coordinate) noise added to them: least squares of 8 parameters on N pairs leaves
    # about sigma * sqrt(8 / 2N) per coordinate, far below sigma for N >= 29.
    pts = r["score"]["pts"][c["planted"]]
    hom = np.concatenate([pts[:, :2], np.ones((len(pts), 1))], 1)
    true = hom @ sp.PLANTED_H.T
    rms = lambda H: np.sqrt((((true[:, :2] / true[:, 2:]) - ((hom @ H.T)[:, :2] / (hom @ H.T)[:, 2:])) ** 2).sum(1).mean())
    assert rms(sp.fit(pts[:, :2], pts[:, 2:], sp.HOMOGRAPHY)) <= 0.3 * np.sqrt(2.0)
    assert rms(r["H"]) <= TH + 0.3 * np.sqrt(2.0)
    assert r["H"][2, 2] == 1.0


@pytest.mark.parametrize("case", CASES)
def test_preconditions_of_the_gpu_tests(cases, case):
    c = cases[case]
    T = case[0]
    sc = c["sc"]
    # 1. few pairs sit within BAND of the threshold, and an fp32 evaluation of the scoring rule never moves a count by more than its band pairs
    assert sc["band"].sum() <= 1e-3 * T * T, sc["band"].sum() / (T * T)
    near = sc["err"] < 2 * TH
    assert np.abs(c["e32"] - sc["err"])[near].max() < sp.BAND / 5, "fp32 vs fp64 sqrt(e): BAND is meant to be 10x this"
    assert (np.abs(c["c32"] - sc["counts"]) <= sc["band"]).all()
    assert (sc["counts"][sc["hyp_ok"]] >= 1).all()
    # 2. no pair within BAND of the threshold in any refit iteration, from the inlier set an fp32 scoring gives (what the device starts from)
    best = sp.select(c["c32"])
    # ... and that inlier set and its hypothesis are the float64 ones, so that the device's refit can be held against the all-float64 restatement
    assert best == sp.select(sc["counts"]) and sc["band"][best] == 0 and np.array_equal(c["inl32"][best], sc["inl"][best])
    for model in (sp.HOMOGRAPHY, sp.AFFINE):
        r = sp.refine(c["l1"], c["l2"], c["tent"], TH, model, 3, best, c["inl32"][best], c["c32"][best])
        assert r["margin"] > sp.BAND, (model, r["margin"])
        assert r["summary"][3] == 0 and r["summary"][2] >= r["summary"][1]


def test_restatement_edge_rules():
    l1, l2, tent, _ = sp.planted(65, 0)
    # lo_iters = 0: the affine hypothesis itself, which maps its own centre exactly
    r = sp.verify(l1, l2, tent, TH, sp.HOMOGRAPHY, 0)
    i, j = tent[r["best"]]
    assert np.allclose(r["H"] @ np.append(l1[i][:, 2].astype(np.float64), 1.0), np.append(l2[j][:, 2].astype(np.float64), 1.0), atol=1e-9)
    assert np.array_equal(r["H"][2], [0, 0, 1]) and r["summary"][2] == r["summary"][1] == r["counts"][r["best"]]
    # every tentative the same pair: all counts T, best 0, coincident points -> degenerate (flag 4)
    same = np.repeat(tent[:1], 9, 0)
    r = sp.verify(l1, l2, same, TH, sp.HOMOGRAPHY, 3)
    assert (r["counts"] == 9).all() and r["summary"] == [0, 9, 9, 4]
    # invalid rows: singular L1, NaN in L2, infinite centre; out-of-range indices
    a, b = l1.copy(), l2.copy()
    a[tent[3, 0], 1, :2] = a[tent[3, 0], 0, :2]
    b[tent[4, 1], 0, 1] = np.nan
    a[tent[5, 0], 0, 2] = np.inf
    t2 = tent.copy()
    t2[6] = (-1, 0)
    t2[7] = (0, len(b))
    sc = sp.score(a, b, t2, TH)
    assert (sc["counts"][[3, 4, 5, 6, 7]] == 0).all() and not sc["hyp_ok"][[3, 4, 5, 6, 7]].any()
    assert not sc["inl"][:, [5, 6, 7]].any(), "a match with a bad index or a non-finite centre is an inlier of nobody"
    assert sc["match_ok"][[3, 4]].all(), "a match whose frame shape is unusable still has usable centres"
    r = sp.verify(a, b, t2[[3, 4, 5, 6, 7]], TH, sp.HOMOGRAPHY, 3)
    assert r["summary"] == [-1, 0, 0, 1]
    # too few inliers: two pairs
    r = sp.verify(l1, l2, np.repeat(tent[:1], 2, 0), TH, sp.HOMOGRAPHY, 3)
    assert r["summary"] == [0, 2, 2, 2]


def test_golden_graf_tentatives_have_too_few_inliers(golden_dir):
    g = np.load(os.path.join(golden_dir, "match_graf16_n500.npz"))
    tent = np.stack([g["tent1"], g["tent2"]], 1).astype(np.int32)
    assert tent.shape == (63, 2)
    r = sp.verify(g["LAFs1"], g["LAFs2"], tent, TH, sp.HOMOGRAPHY, 3)
    assert r["summary"][1] == 3 and r["summary"][3] == 2, r["summary"]
    assert np.array_equal(r["H"], sp.hypothesis_model(g["LAFs1"], g["LAFs2"], tent[r["best"]]))


def test_scratch_bytes_and_symbols():
    from affnet_amd import _lib
    f = _lib.lib.affnet_verify_scratch_bytes
    sizes = [f(t) for t in (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 2000, 100000)]
    assert sizes[1] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] >= 100000 * 33, "two float4 and one mask byte per row"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "affnet_hip.h")).read(), flags=re.S)
    for name, nargs in (("affnet_verify_scratch_bytes", 1), ("affnet_verify_score", 13), ("affnet_verify_matches", 17)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define\s+AFFNET_VERIFY_TILE\s+%d\b" % _lib.VERIFY_TILE, hdr) and re.search(r"#define\s+AFFNET_VERIFY_CHUNK\s+%d\b" % _lib.VERIFY_CHUNK, hdr)
    assert re.search(r"#define\s+AFFNET_VERIFY_AFFINE\s+0\b", hdr) and re.search(r"#define\s+AFFNET_VERIFY_HOMOGRAPHY\s+1\b", hdr)


def test_bad_arguments_are_refused_before_any_device_work():
    """The argument checks run on the host, in front of the first launch: they need no GPU."""
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        p = C.c_void_p(4096)            # never dereferenced: every call below is refused
        ok = dict(l1=p, n1=4, l2=p, n2=4, tent=p, count=None, t=4, th=3.0, model=1, it=3, counts=p, H=p, inl=p, summ=p, scr=p)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.affnet_verify_matches(h, a["l1"], a["n1"], a["l2"], a["n2"], a["tent"], a["count"], a["t"], a["th"], a["model"], a["it"], a["counts"],
                                             a["H"], a["inl"], a["summ"], a["scr"], None)
        bad = [dict(l1=None), dict(l2=None), dict(tent=None), dict(counts=None), dict(H=None), dict(inl=None), dict(summ=None), dict(scr=None), dict(t=-1),
               dict(th=0.0), dict(th=-1.0), dict(th=float("nan")), dict(th=float("inf")), dict(model=2), dict(model=-1), dict(it=-1), dict(it=9),
               dict(scr=C.c_void_p(4100))]
        for kw in bad:
            assert call(**kw) == _lib.ERR_INVALID, kw
            assert b"verify_matches" in lib.affnet_last_error(h), kw
        assert lib.affnet_verify_score(h, p, 4, p, 4, p, None, 4, 3.0, p, None, p, None) == _lib.ERR_INVALID
        assert lib.affnet_verify_score(h, p, 4, p, 4, p, None, 4, float("nan"), p, p, p, None) == _lib.ERR_INVALID
        assert b"verify_score" in lib.affnet_last_error(h)
    finally:
        lib.affnet_ctx_destroy(h)


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import ReprojectionStuff as RS
    for name in ("verify_matches", "enqueue_verify", "match_and_verify"):
        assert getattr(affnet_amd, name) is getattr(RS, name)
    with pytest.raises(RuntimeError):
        RS.verify_matches(np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), [0], [0])        # no CPU path
