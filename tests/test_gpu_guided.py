"""MI355X: guided matching (csrc/guided.hip: affnet_match_guided, affnet_guided_mask; ReprojectionStuff.match_guided, guided_mask,
match_verify_guided) against its float32 restatement tests/_guided_fp32.py, which tests/test_guided_host.py pins.  Comparisons are on the bytes
unless a band is stated."""
import os

import numpy as np
import pytest
import torch

import _epipolar_fp64 as ep
import _guided_fp32 as gf
import _match_fp32 as mf
import _spatial_fp64 as sp
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_I32, SENT_F32, SENT_U8 = -7, -12345.0, 0xAB
INF = float("inf")
MASK_SHAPES = [(1, 1), (15, 16), (17, 33), (65, 200), (130, 415)]
# (1025, 200): the selection works in rounds of 1024 rows
DENSE_SHAPES = mf.MATRIX_SHAPES + [(1025, 200)]
REPEATED = [65, 130, 257]
KINDS = {gf.PLANAR: "planar", gf.EPIPOLAR: "epipolar"}


def _dev(x, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(DEV)          # a copy: the scenes are read-only


def raw_mask(l1, l2, model, kind, r):
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    a, b, m = _dev(l1, np.float32), _dev(l2, np.float32), _dev(np.asarray(model, np.float64).reshape(9), np.float64)
    n1, n2 = a.size(0), b.size(0)
    mask = torch.full((n1 * n2 + 16,), SENT_U8, dtype=torch.uint8, device=dev)
    scratch = torch.empty(lib.affnet_match_guided_scratch_bytes(n1, n2, 1), dtype=torch.uint8, device=dev)
    ctx = engine.utility_ctx(dev)
    check(lib.affnet_guided_mask(ctx, ptr(a), n1, ptr(b), n2, ptr(m), kind, r, ptr(mask), ptr(scratch), engine.stream_of(dev)), ctx, "affnet_guided_mask")
    torch.cuda.synchronize()
    out = mask.cpu().numpy()
    assert (out[n1 * n2:] == SENT_U8).all(), "nothing behind the matrix is written"
    return out[:n1 * n2].reshape(n1, n2)


def raw_guided(d1, d2, l1, l2, model, kind, r, thr, max_dist=INF, mutual=True, n_chunks=0, gate=None, dim=128, n1=None, n2=None, flags=None, null=None,
               want_rc=0):
    """affnet_match_guided on buffers of this test, pre-filled with sentinels so that "not written" can be seen -> dict of numpy arrays.
    null: the name of one pointer argument to pass as NULL; want_rc: the return code the call must give."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr
    dev = torch.device(DEV)
    t = dict(d1=_dev(d1, np.float32), d2=_dev(d2, np.float32), l1=_dev(l1, np.float32), l2=_dev(l2, np.float32),
             model=_dev(np.asarray(model, np.float64).reshape(9), np.float64))
    N1 = t["d1"].size(0) if n1 is None else n1
    N2 = t["d2"].size(0) if n2 is None else n2
    cap = max(t["d1"].size(0), 1)
    t["dist"] = torch.full((cap, 2), SENT_F32, dtype=torch.float32, device=dev)
    t["idx"] = torch.full((cap, 2), SENT_I32, dtype=torch.int32, device=dev)
    t["tent"] = torch.full((cap, 2), SENT_I32, dtype=torch.int32, device=dev)
    t["count"] = torch.full((1,), SENT_I32, dtype=torch.int32, device=dev)
    t["scratch"] = torch.empty(lib.affnet_match_guided_scratch_bytes(max(N1, 0), max(N2, 0), min(max(n_chunks, 0), 65535)), dtype=torch.uint8, device=dev)
    p = {k: (None if k == null else ptr(v)) for k, v in t.items()}
    ctx = None if null == "ctx" else engine.utility_ctx(dev)
    fl = (1 if mutual else 0) if flags is None else flags
    rc = lib.affnet_match_guided(ctx, p["d1"], N1, p["d2"], N2, dim, p["l1"], p["l2"], p["model"], kind, r, thr, max_dist, fl, n_chunks,
                                 None if gate is None else ptr(gate), p["dist"], p["idx"], p["tent"], p["count"], p["scratch"], engine.stream_of(dev))
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, want_rc)
    return {k: t[k].cpu().numpy() for k in ("dist", "idx", "tent", "count")}


def check_against(got, want, n1, what):
    assert np.array_equal(got["dist"][:n1].view(np.uint32), want["dist"].view(np.uint32)), (what, "dist", np.nonzero((got["dist"][:n1].view(np.uint32) != want["dist"].view(np.uint32)).any(1))[0][:8])
    assert np.array_equal(got["idx"][:n1], want["idx"]), (what, "idx", np.nonzero((got["idx"][:n1] != want["idx"]).any(1))[0][:8])
    k = want["count"]
    assert got["count"][0] == k, (what, "count", int(got["count"][0]), k)
    assert np.array_equal(got["tent"][:k], want["tent"]), (what, "tent")
    assert (got["tent"][k:] == SENT_I32).all(), (what, "rows at or beyond the count are not written")


def scene_of(name, arg, kind):
    """-> (scene dict, model, radius, distance matrix, admissible matrix), computed once per scene."""
    if name == "dense":
        sc = gf.dense_scene(*arg)
        model, r = (sc["model"], gf.DENSE_R) if kind == gf.PLANAR else (ep.planted_F().reshape(3, 3), gf.DENSE_R)
        M = gf.scene_distance(("dense",) + tuple(arg), sc)
    else:
        sc = gf.repeated_scene(arg, arg, kind)
        model, r = sc["model"], (10.0 if kind == gf.PLANAR else 4.0)
        M = gf.scene_distance(("rep", arg, kind), sc)
    return sc, model, r, M, gf.admissible(sc["l1"], sc["l2"], model, kind, r)


# ---- mask ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", MASK_SHAPES)
def test_mask_is_the_restatement(shape, kind):
    sc, model, r, _, adm = scene_of("dense", shape, kind)
    got = raw_mask(sc["l1"], sc["l2"], model, kind, r)
    assert np.array_equal(got, adm.astype(np.uint8)), np.argwhere(got != adm)[:8]


def test_mask_on_the_boundary_pairs():
    l1, l2 = gf.boundary_pairs()
    for model, kind in ((np.eye(3), gf.PLANAR), (gf.NEG_W, gf.PLANAR), (np.zeros((3, 3)), gf.EPIPOLAR), (np.eye(3), gf.EPIPOLAR)):
        got = raw_mask(l1, l2, model, kind, 5.0)
        assert np.array_equal(got, gf.admissible(l1, l2, model, kind, 5.0).astype(np.uint8)), (model, kind)
    eye = raw_mask(l1, l2, np.eye(3), gf.PLANAR, 5.0)
    assert eye.tolist() == [[1, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert not raw_mask(l1, l2, gf.NEG_W, gf.PLANAR, 5.0).any() and not raw_mask(l1, l2, np.zeros((3, 3)), gf.EPIPOLAR, 5.0).any()
    # the Python wrapper is the same call
    from affnet_amd import ReprojectionStuff as RS
    m = RS.guided_mask(_dev(l1, np.float32), _dev(l2, np.float32), torch.eye(3, dtype=torch.float64), "homography", 5.0)
    assert m.dtype == torch.bool and np.array_equal(m.cpu().numpy(), eye.astype(bool))


# ---- the lists and the selection ---------------------------------------------------------------------------------------------------------
def _sweep(name, arg, kind):
    sc, model, r, M, adm = scene_of(name, arg, kind)
    n1 = sc["d1"].shape[0]
    base = gf.guided_from(M, adm, 1.0, mutual=False)
    finite = np.sort(base["dist"][:, 0][np.isfinite(base["dist"][:, 0])])
    cut = float(finite[len(finite) // 2]) if len(finite) else 1.0            # a distance that occurs: rows AT max_dist are kept
    kept = []
    for mutual in (True, False):
        for max_dist in (INF, cut):
            for thr in (0.8, 0.9, 1.0):
                want = gf.guided_from(M, adm, thr, max_dist, mutual)
                got = raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, kind, r, thr, max_dist, mutual)
                check_against(got, want, n1, (name, arg, kind, mutual, max_dist, thr))
                kept.append(want["count"])
    return sc, model, r, base, kept


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_scene_lists_and_selection(shape, kind):
    _, _, _, base, kept = _sweep("dense", shape, kind)
    if shape[1] >= 40 and shape[0] >= 23:
        assert len(set(kept)) > 3, "the flags, the bound and the thresholds each change what is kept"
        assert (base["idx"][:, 1] >= 0).any() and (kind == gf.EPIPOLAR or np.isnan(base["dist"]).any())


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("T", REPEATED)
def test_repeated_scene_lists_and_selection(T, kind):
    sc, model, r, base, kept = _sweep("rep", T, kind)
    # validity: every kept pair lies within the radius, by the float64 distance, up to the band of the fp32 test
    got = raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, kind, r, 0.9)
    k = int(got["count"][0])
    tent = got["tent"][:k]
    pts = np.stack([sc["l1"][tent[:, 0], 0, 2], sc["l1"][tent[:, 0], 1, 2], sc["l2"][tent[:, 1], 0, 2], sc["l2"][tent[:, 1], 1, 2]], 1).astype(np.float64)
    m32 = np.asarray(model, np.float64).astype(np.float32).astype(np.float64)
    dist = sp.transfer(m32.reshape(3, 3), pts)[0] if kind == gf.PLANAR else ep.sampson(m32.reshape(9), pts)
    band = gf.PLANAR_BAND if kind == gf.PLANAR else ep.BAND
    planted = sc["partner"] >= 0
    true = int((sc["partner"][tent[:, 0]] == tent[:, 1]).sum())
    print("repeated scene T=%d %s: kept %d, planted %d, true %d, largest float64 distance %.4f px (radius %g, band %.3g)" % (
        T, KINDS[kind], k, planted.sum(), true, dist.max(), r, band))
    record_parity("guided matching, repeated scene T = %d, %s" % (T, KINDS[kind]), kept=k, planted=int(planted.sum()), true=true,
                  largest_distance_px=float(dist.max()), radius_px=r, band_px=band)
    assert dist.max() <= r + band and true == planted.sum()


@pytest.mark.parametrize("kind", list(KINDS))
def test_result_does_not_depend_on_the_chunks(kind):
    sc, model, r, M, adm = scene_of("dense", (130, 415), kind)
    want = gf.guided_from(M, adm, 0.9, INF, True)
    for nc in (0, 1, 2, 3, 7, 40):                   # 415 columns are 26 tiles, 130 rows are 9
        check_against(raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, kind, r, 0.9, n_chunks=nc), want, 130, (kind, nc))


def test_everything_admitted_is_knn_and_match_snn():
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    n1, n2 = 130, 415
    q, db = mf.planted(n1, n2)
    l1, l2 = np.zeros((n1, 2, 3), np.float32), np.zeros((n2, 2, 3), np.float32)
    l1[:, :, 2] = l2[:, :, 2] = (50.0, 60.0)
    got = raw_guided(q, db, l1, l2, np.eye(3), gf.PLANAR, 1.0, 1.0, mutual=False)
    a, b = _dev(q, np.float32), _dev(db, np.float32)
    kd = torch.empty(n1, 2, dtype=torch.float32, device=dev)
    ki = torch.empty(n1, 2, dtype=torch.int32, device=dev)
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    scratch = torch.empty(lib.affnet_knn_scratch_bytes(n1, n2, 2, 0), dtype=torch.uint8, device=dev)
    check(lib.affnet_knn(ctx, ptr(a), n1, ptr(b), n2, 128, 2, 0, 0, 0, ptr(kd), ptr(ki), ptr(scratch), st), ctx, "affnet_knn")
    md, md2 = torch.empty(n1, device=dev), torch.empty(n1, device=dev)
    mi = torch.empty(n1, dtype=torch.int32, device=dev)
    tent, cnt = torch.empty(n1, 2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    scratch2 = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=dev)
    check(lib.affnet_match_snn(ctx, ptr(a), n1, ptr(b), n2, 128, 0.8, ptr(md), ptr(mi), ptr(md2), ptr(tent), ptr(cnt), ptr(scratch2), st), ctx, "affnet_match_snn")
    torch.cuda.synchronize()
    assert np.array_equal(got["dist"].view(np.uint32), kd.cpu().numpy().view(np.uint32)) and np.array_equal(got["idx"], ki.cpu().numpy())
    assert np.array_equal(got["dist"][:, 0].view(np.uint32), md.cpu().numpy().view(np.uint32)) and np.array_equal(got["idx"][:, 0], mi.cpu().numpy())
    assert np.isnan(got["dist"]).any()


def test_epipolar_mask_is_the_verification_scoring():
    from affnet_amd import ReprojectionStuff as RS
    l1, l2, tent, _, _ = ep.planted_two_view(128, 0.5, 128)
    L1, L2 = _dev(l1, np.float32), _dev(l2, np.float32)
    th = 2.0
    F, inl, info = RS.verify_epipolar(L1, L2, torch.from_numpy(tent[:, 0].copy()), torch.from_numpy(tent[:, 1].copy()), th)
    assert info["flags"] == 0
    mask = RS.guided_mask(L1, L2, F, "fundamental", th).cpu().numpy()
    F32 = F.cpu().numpy().reshape(1, 9).astype(np.float32)
    want = ep.score_fp32(F32, ep.gather(l1, l2, tent)[0], th)[1][0]
    assert np.array_equal(mask[tent[:, 0], tent[:, 1]], want) and 8 <= want.sum() < 128


def test_closed_gate_matches_nothing():
    from affnet_amd import ReprojectionStuff as RS
    for kind in KINDS:
        sc, model, r, M, adm = scene_of("dense", (65, 200), kind)
        L1, L2 = _dev(sc["l1"], np.float32), _dev(sc["l2"], np.float32)
        empty = torch.zeros(0, 2, dtype=torch.int32, device=DEV)
        H, _, _, summary = RS.enqueue_verify(L1, L2, empty) if kind == gf.PLANAR else RS.enqueue_verify_epipolar(L1, L2, empty)
        assert summary.cpu().tolist() == [-1, 0, 0, 1]
        for mutual in (True, False):
            got = raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, kind, r, 1.0, mutual=mutual, gate=summary)
            check_against(got, gf.guided_from(M, adm, 1.0, INF, mutual, closed=True), 65, (kind, mutual))
            assert got["count"][0] == 0 and (got["idx"] == -1).all() and np.isinf(got["dist"]).all() and (got["tent"] == SENT_I32).all()
        opened = torch.tensor([3, 9, 9, 2], dtype=torch.int32, device=DEV)          # other flags do not close it
        check_against(raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, kind, r, 1.0, gate=opened), gf.guided_from(M, adm, 1.0), 65, (kind, "open"))


def test_empty_sides():
    sc, model, r, _, _ = scene_of("dense", (17, 33), gf.PLANAR)
    got = raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, gf.PLANAR, r, 1.0, n2=0)
    assert got["count"][0] == 0 and (got["idx"] == -1).all() and np.isinf(got["dist"]).all() and (got["tent"] == SENT_I32).all()
    got = raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, gf.PLANAR, r, 1.0, n1=0)
    assert got["count"][0] == 0 and (got["idx"] == SENT_I32).all() and (got["tent"] == SENT_I32).all()


def test_refused_arguments_leave_the_buffers_alone():
    from affnet_amd import _lib
    sc, model, r, _, _ = scene_of("dense", (17, 33), gf.PLANAR)
    base = dict(kind=gf.PLANAR, r=r, thr=0.9)
    bad = [dict(dim=64), dict(kind=2), dict(kind=-1), dict(flags=2), dict(flags=3), dict(r=0.0), dict(r=-1.0), dict(r=INF), dict(r=float("nan")),
           dict(max_dist=float("nan")), dict(n1=-1), dict(n2=-1), dict(n_chunks=-1), dict(n_chunks=65536)]
    bad += [dict(null=k) for k in ("ctx", "d1", "d2", "l1", "l2", "model", "dist", "idx", "tent", "count", "scratch")]
    for kw in bad:
        got = raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, want_rc=_lib.ERR_INVALID, **dict(base, **kw))
        assert (got["dist"] == SENT_F32).all() and (got["idx"] == SENT_I32).all() and (got["tent"] == SENT_I32).all() and got["count"][0] == SENT_I32, kw
    # the same values that are valid
    for kw in (dict(n_chunks=65535), dict(max_dist=-INF), dict(flags=0)):
        raw_guided(sc["d1"], sc["d2"], sc["l1"], sc["l2"], model, **dict(base, **kw))


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["homography", "affine", "fundamental"])
def test_chain_is_the_four_calls(model):
    from affnet_amd import ReprojectionStuff as RS
    kind = gf.EPIPOLAR if model == "fundamental" else gf.PLANAR
    sc = gf.repeated_scene(257, 257, kind)
    D1, D2, L1, L2 = (_dev(sc[k], np.float32) for k in ("d1", "d2", "l1", "l2"))
    th = 3.0
    t1, t2, H, inl, info = RS.match_verify_guided(D1, D2, L1, L2, 0.8, th, model, seed=3)
    m1, m2, _, _ = RS.match_snn(D1, D2, 0.8)
    H0, inl0, info0 = RS.verify_matches(L1, L2, m1, m2, th, model, 3, seed=3)
    g1, g2, dist, idx = RS.match_guided(D1, D2, L1, L2, H0, model, None, 0.9)
    H1, inl1, info1 = RS.verify_matches(L1, L2, g1, g2, th, model, 3, seed=3)
    assert torch.equal(t1, g1) and torch.equal(t2, g2) and torch.equal(H, H1) and torch.equal(inl, inl1) and torch.equal(info["counts"], info1["counts"])
    seed_stage = info.pop("seed_stage")
    assert {k: v for k, v in info.items() if k != "counts"} == {k: v for k, v in info1.items() if k != "counts"}
    assert seed_stage == {"tentatives": m1.numel(), "num_inliers": info0["num_inliers"], "flags": info0["flags"]} and info0["flags"] == 0
    assert t1.dtype == torch.int64 and dist.shape == (257, 2) and idx.dtype == torch.int32
    # every guided tentative is admissible under the seed model
    radius = 10.0 if kind == gf.PLANAR else 4.0
    assert RS.guided_mask(L1, L2, H0, model, radius)[t1, t2].all()
    planted = np.nonzero(sc["partner"] >= 0)[0]
    final = set(zip(t1[inl].tolist(), t2[inl].tolist()))
    have = sum((int(i), int(sc["partner"][i])) in final for i in planted)
    print("chain %s: seed tentatives %d, inliers %d -> guided tentatives %d, inliers %d; planted rows %d, among the final inliers %d" % (
        model, m1.numel(), info0["num_inliers"], t1.numel(), info["num_inliers"], len(planted), have))
    record_parity("match_verify_guided, repeated scene T = 257, %s" % model, seed_tentatives=int(m1.numel()), seed_inliers=info0["num_inliers"],
                  guided_tentatives=int(t1.numel()), guided_inliers=info["num_inliers"], planted=int(len(planted)), planted_among_inliers=int(have))
    assert info["num_inliers"] >= info0["num_inliers"]
    if model == "homography":
        assert have == len(planted), "the final inliers contain every planted row"


def test_chain_without_a_model_is_empty():
    from affnet_amd import ReprojectionStuff as RS
    rng = np.random.default_rng(1)
    d = rng.normal(size=(40, 128)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    l = np.full((40, 2, 3), np.nan, np.float32)                # no usable frame: no valid hypothesis
    D, L = _dev(d, np.float32), _dev(l, np.float32)
    for model in ("homography", "fundamental"):
        t1, t2, H, inl, info = RS.match_verify_guided(D, D, L, L, 0.8, 3.0, model)
        assert t1.numel() == 0 and t2.numel() == 0 and inl.numel() == 0 and info["flags"] & 1 and info["seed_stage"]["flags"] & 1
        assert info["seed_stage"]["tentatives"] > 0 and info["num_inliers"] == 0
    with pytest.raises(ValueError):
        RS.match_verify_guided(D, D, L, L[:5])
    with pytest.raises(ValueError):
        RS.match_guided(D, D[:0], L, L[:0], torch.eye(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        RS.match_guided(D, D, L, L, torch.eye(3, dtype=torch.float64), kind="similarity")


def test_graf_1_6():
    from affnet_amd import ReprojectionStuff as RS
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_graf16_n500.npz"))
    D1, D2, L1, L2 = _dev(g["desc1"], np.float32), _dev(g["desc2"], np.float32), _dev(g["LAFs1"], np.float32), _dev(g["LAFs2"], np.float32)
    Hgt = torch.from_numpy(g["H"])

    def consistent(t1, t2):
        return int(RS.get_GT_correspondence_indexes(L1[t1], L2[t2], Hgt, dist_threshold=6)[1].numel()) if t1.numel() else 0
    p1, p2, H0, inl0, info0 = RS.match_and_verify(D1, D2, L1, L2, 0.8, 3.0, "homography")
    t1, t2, H, inl, info = RS.match_verify_guided(D1, D2, L1, L2, 0.8, 3.0, "homography")
    assert info["seed_stage"] == {"tentatives": p1.numel(), "num_inliers": info0["num_inliers"], "flags": info0["flags"]}
    assert t1.numel() == 0 or RS.guided_mask(L1, L2, H0, "homography")[t1, t2].all()
    rec = dict(plain_tentatives=int(p1.numel()), plain_inliers=info0["num_inliers"], plain_consistent=consistent(p1, p2),
               plain_inliers_consistent=consistent(p1[inl0], p2[inl0]), guided_tentatives=int(t1.numel()), guided_inliers=info["num_inliers"],
               guided_consistent=consistent(t1, t2), guided_inliers_consistent=consistent(t1[inl], t2[inl]), seed_flags=info0["flags"], flags=info["flags"])
    print("graf 1-6, SIFT, 500 kp:", rec)
    record_parity("guided matching graf 1-6, SIFT slot, 500 kp, homography", **rec)
