"""CPU: pins tests/_guided_fp32.py, the restatement tests/test_gpu_guided.py compares the guided-matching kernels with, to restatements the
project already trusts (_match_fp32, _spatial_fp64, _epipolar_fp64), and proves that its scenes contain what they claim."""
import numpy as np
import pytest

import _epipolar_fp64 as ep
import _guided_fp32 as gf
import _match_fp32 as mf
import _spatial_fp64 as sp

REPEATED = [65, 130, 257]
DENSE = [(65, 200), (200, 415)]


@pytest.mark.parametrize("shape", [(17, 33), (65, 200)])
def test_everything_admitted_is_the_sorted_distance_row(shape):
    q, db = mf.planted(*shape)
    M = mf.distance(q, db)
    g = gf.guided_from(M, np.ones(M.shape, bool), 1.0, mutual=False)
    md, idx = mf.row_min(M)
    assert np.array_equal(g["dist"][:, 0], md, equal_nan=True) and np.array_equal(g["idx"][:, 0], idx)
    for i in range(shape[0]):
        row = M[i]
        nan = np.nonzero(np.isnan(row))[0]
        rest = np.nonzero(~np.isnan(row))[0]
        order = np.concatenate([nan, rest[np.argsort(row[rest], kind="stable")]])[:2]          # stable: the smaller column first among equals
        assert np.array_equal(g["idx"][i], order) and np.array_equal(g["dist"][i], row[order], equal_nan=True), i
    if shape[1] >= 40:
        assert np.isnan(g["dist"][shape[0] - 2]).all(), "the copy of the long row sees NaN columns first"
    # the columns' order is the rows' order of the transposed matrix
    bd, bi = mf.row_min(M.T)
    assert np.array_equal(g["back"], bi)


def _planar_spread(sc, r):
    e32, _ = gf.planar_error(sc["l1"], sc["l2"], sc["model"], np.float32)
    e64, _ = gf.planar_error(sc["l1"], sc["l2"], sc["model"], np.float64)
    with np.errstate(all="ignore"):
        s32, s64 = np.sqrt(e32.astype(np.float64)), np.sqrt(e64)
        near = s64 < 2 * r
    return float(np.abs(s32 - s64)[near].max()), s32, s64


def test_band_is_ten_times_the_fp32_spread():
    worst = 0.0
    for T in REPEATED:
        worst = max(worst, _planar_spread(gf.repeated_scene(T, T), 10.0)[0])
    for shape in DENSE:
        worst = max(worst, _planar_spread(gf.dense_scene(*shape), gf.DENSE_R)[0])
    print("largest |sqrt(e32) - sqrt(e64)| below 2 r: %.3g px, band %.3g px" % (worst, gf.PLANAR_BAND))
    assert 10 * worst <= gf.PLANAR_BAND < 10.2 * worst


@pytest.mark.parametrize("scene", [("rep", T) for T in REPEATED] + [("dense", s) for s in DENSE])
def test_planar_predicate_in_float32_is_within_the_band_of_float64(scene):
    sc, r = (gf.repeated_scene(scene[1], scene[1]), 10.0) if scene[0] == "rep" else (gf.dense_scene(*scene[1]), gf.DENSE_R)
    _, s32, s64 = _planar_spread(sc, r)
    adm = gf.admissible(sc["l1"], sc["l2"], sc["model"], gf.PLANAR, r)
    w64 = gf.planar_error(sc["l1"], sc["l2"], sc["model"], np.float64)[1]
    assert (w64 > 0.5).all()
    diff = adm != (s64 <= r)
    assert not (diff & (np.abs(s64 - r) >= gf.PLANAR_BAND)).any()
    assert np.array_equal(adm, s32 <= r) or np.abs(s32 - r).min() < 1e-6


@pytest.mark.parametrize("kind", [gf.PLANAR, gf.EPIPOLAR])
@pytest.mark.parametrize("T", REPEATED)
def test_repeated_scene_is_what_guided_matching_is_for(T, kind):
    sc = gf.repeated_scene(T, T, kind)
    r = 10.0 if kind == gf.PLANAR else 4.0
    M = gf.scene_distance(("rep", T, kind), sc)
    planted = sc["partner"] >= 0
    rep = sc["repeated"]
    # the decoys are where the docstring says
    pts = np.stack([sc["l1"][rep, 0, 2], sc["l1"][rep, 1, 2], sc["l2"][sc["decoy"][rep], 0, 2], sc["l2"][sc["decoy"][rep], 1, 2]], 1).astype(np.float64)
    far = sp.transfer(sc["model"], pts)[0] if kind == gf.PLANAR else ep.sampson(sc["model"].reshape(9), pts)
    assert (far > (100.0 if kind == gf.PLANAR else 50.0)).all() and rep.sum() == (planted.sum() + 2) // 3
    g = gf.guided_from(M, gf.admissible(sc["l1"], sc["l2"], sc["model"], kind, r), 0.9, mutual=True)
    got = dict(g["tent"].tolist())
    true = [i for i in np.nonzero(planted)[0] if got.get(int(i)) == sc["partner"][i]]
    assert len(true) == planted.sum(), "the guided rule keeps every planted row with its planted partner"
    snn = dict(mf.match_from_matrix(M, 0.8)["tent"].tolist())
    snn_true = [i for i in np.nonzero(planted)[0] if snn.get(int(i)) == sc["partner"][i]]
    snn_rep = [i for i in snn_true if rep[i]]
    print("T=%d kind=%d: planted %d, repeated %d | match_snn true %d, on repeated %d | guided true %d, on repeated %d, other pairs %d" % (
        T, kind, planted.sum(), rep.sum(), len(snn_true), len(snn_rep), len(true), int(rep[true].sum()), g["count"] - len(true)))
    assert 2 * len(snn_rep) < rep.sum(), "match_snn keeps fewer than half of the repeated rows"


@pytest.mark.parametrize("shape", DENSE)
def test_dense_scene_contains_the_claimed_cases(shape):
    sc = gf.dense_scene(*shape)
    n1, n2 = shape
    assert (sc["l2"][:, :, 2] >= 0).all() and (sc["l2"][:, :, 2] <= 120).all()
    M = gf.scene_distance(("dense",) + shape, sc)
    adm = gf.admissible(sc["l1"], sc["l2"], sc["model"], gf.PLANAR, gf.DENSE_R)
    per_row = adm.sum(1)
    assert per_row[1] == 0 and per_row[2] == 1 and adm[2, 3] and (per_row >= 2).sum() > n1 // 2 and np.median(per_row) >= 16
    g = gf.guided_from(M, adm, 1.0, mutual=False)
    assert g["idx"][0].tolist() == [5, 21] and g["dist"][0, 0] == g["dist"][0, 1], "a row whose two best admissible columns tie"
    assert np.isnan(g["dist"][n1 - 2, 0]) and g["idx"][n1 - 2, 0] == 0 and not g["keep"][n1 - 2], "a NaN nearest admissible distance, refused"
    assert g["idx"][1].tolist() == [-1, -1] and np.isinf(g["dist"][1]).all() and g["idx"][2].tolist() == [3, -1] and g["keep"][2], "ratio 0 with one column"
    for thr in (0.8, 0.9, 1.0):
        a, b = gf.guided_from(M, adm, thr, mutual=False), gf.guided_from(M, adm, thr, mutual=True)
        assert b["count"] < a["count"] and (a["keep"] | ~b["keep"]).all(), "a match that the mutual test alone removes (thr %g)" % thr
    # the admissible set changes the answer: some row's nearest admissible column is not its nearest column
    assert (g["idx"][:, 0] != mf.row_min(M)[1]).sum() > n1 // 4
    # the epipolar kind on the same frames admits a wide band: most rows have many admissible columns, some pairs are refused
    adm_e = gf.admissible(sc["l1"], sc["l2"], ep.planted_F(), gf.EPIPOLAR, gf.DENSE_R)
    assert 0.2 < adm_e.mean() < 0.999 and (adm_e.sum(1) >= 2).mean() > 0.9


def test_boundary_pairs():
    l1, l2 = gf.boundary_pairs()
    eye = np.eye(3)
    adm = gf.admissible(l1, l2, eye, gf.PLANAR, 5.0)
    want = np.zeros((5, 3), bool)
    want[0, 0] = want[0, 2] = True                  # (3, 4): 25 <= 25; one ulp further is not; the point itself
    assert np.array_equal(adm, want)
    neg = gf.admissible(l1, l2, gf.NEG_W, gf.PLANAR, 5.0)
    e, W = gf.planar_error(l1, l2, gf.NEG_W)
    assert e[1, 2] == 0 and W[1] == -1 and not neg.any(), "W <= 0 admits nothing, although the point lands on a column"
    assert not gf.admissible(l1, l2, np.zeros((3, 3)), gf.EPIPOLAR, 5.0).any(), "an all-zero F admits nothing"
    bad = eye.copy()
    bad[0, 1] = np.inf
    assert not gf.admissible(l1, l2, bad, gf.PLANAR, 5.0).any() and not gf.admissible(l1, l2, bad, gf.EPIPOLAR, 5.0).any()
    # the epipolar tree on a real F agrees with the scoring restatement at the tentatives
    a, b, tent, _, F = ep.planted_two_view(64, 0.5, 3)
    pts = ep.gather(a, b, tent)[0]
    inl = ep.score_fp32(F.reshape(1, 9).astype(np.float32), pts, 2.0)[1][0]
    assert np.array_equal(gf.admissible(a, b, F, gf.EPIPOLAR, 2.0)[tent[:, 0], tent[:, 1]], inl)
    # a closed gate leaves everything unfilled
    g = gf.guided_from(np.ones((5, 3), np.float32), adm, 1.0, closed=True)
    assert g["count"] == 0 and (g["idx"] == -1).all() and np.isinf(g["dist"]).all() and (g["back"] == -1).all()
