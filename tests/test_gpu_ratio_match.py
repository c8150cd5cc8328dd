"""MI355X: ratio-test matching (affnet_match_ratio, affnet_match_ratio_many; ReprojectionStuff.match_ratio / match_fginn and matcher="snn" /
"fginn" of the match-and-verify chains) against tests/_ratio_fp32.py, the float32 restatement that tests/test_ratio_mirror_host.py pins, against
the device code the project already has (affnet_knn, affnet_distance_matrix), and the many-pairs call and the chains against the single-pair
calls.  Every distance is the element affnet_distance_matrix writes and the order of candidates is total, so the tolerance is zero: every
comparison below is on the bytes."""
import numpy as np
import pytest
import torch

import _guided_fp32 as gf
import _match_fp32 as mf
import _ratio_fp32 as rf
import _spatial_fp64 as sp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = float("inf")
THR = 0.8
SENT_F32, SENT_I32 = -7.5, -7
RADII = (-1.0, 0.0, 10.0)
CHUNKS = (0, 1, 2, 3, 7)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _api():
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    return lib, ptr, check, engine.utility_ctx(dev), engine.stream_of(dev), dev


def full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def dev_of(x, dtype=np.float32):
    return torch.from_numpy(np.array(x, dtype)).to(DEV)          # a copy: the scenes are read-only


def _stand_in(t):
    return t if t.numel() else torch.zeros(8, dtype=torch.float32, device=DEV)          # never read, but the boundary refuses NULL


# ---- the raw calls, on buffers pre-filled with sentinels so that "not written" can be seen ---------------------------------------------------
def raw_ratio(d1, d2, l2, r, thr=THR, max_dist=INF, mutual=False, n_chunks=0):
    """affnet_match_ratio on device tensors -> numpy dict; tent rows at and beyond the count hold the sentinel."""
    lib, ptr, check, ctx, st, dev = _api()
    n1, n2 = d1.size(0), d2.size(0)
    dist, idx = full((max(n1, 1), 2), SENT_F32, torch.float32), full((max(n1, 1), 2), SENT_I32, torch.int32)
    tent, cnt = full((max(n1, 1), 2), SENT_I32, torch.int32), full((1,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_match_ratio_scratch_bytes(n1, n2, n_chunks), dtype=torch.uint8, device=dev)
    check(lib.affnet_match_ratio(ctx, ptr(_stand_in(d1)), n1, ptr(_stand_in(d2)), n2, 128, None if l2 is None else ptr(_stand_in(l2)), r, thr, max_dist,
                                 1 if mutual else 0, n_chunks, ptr(dist), ptr(idx), ptr(tent), ptr(cnt), ptr(scratch), st), ctx, "affnet_match_ratio")
    return dict(dist=dist.cpu().numpy()[:n1], idx=idx.cpu().numpy()[:n1], tent=tent.cpu().numpy()[:n1], count=int(cnt.item()))


def raw_ratio_many(D1, D2, L2, table, n1_max, n2_max, r, thr=THR, max_dist=INF, mutual=False, n_chunks=0):
    lib, ptr, check, ctx, st, dev = _api()
    P = table.shape[0]
    dist, idx = full((P, max(n1_max, 1), 2), SENT_F32, torch.float32), full((P, max(n1_max, 1), 2), SENT_I32, torch.int32)
    tent, cnt = full((P, max(n1_max, 1), 2), SENT_I32, torch.int32), full((P,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_match_ratio_many_scratch_bytes(P, n1_max, n2_max, n_chunks), dtype=torch.uint8, device=dev)
    pairs = torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev)
    check(lib.affnet_match_ratio_many(ctx, ptr(D1), D1.size(0), ptr(D2), D2.size(0), 128, None if L2 is None else ptr(L2), ptr(pairs), P, n1_max, n2_max, r, thr,
                                      max_dist, 1 if mutual else 0, n_chunks, ptr(dist), ptr(idx), ptr(tent), ptr(cnt), ptr(scratch), st), ctx,
          "affnet_match_ratio_many")
    return dict(dist=dist.cpu().numpy(), idx=idx.cpu().numpy(), tent=tent.cpu().numpy(), count=cnt.cpu().numpy())


def check_against_mirror(got, want, n1, what):
    assert same(got["dist"], want["dist"]), what
    assert same(got["idx"], want["idx"]), what
    assert got["count"] == want["count"], what
    assert same(got["tent"][:want["count"]], want["tent"]), what
    assert (got["tent"][want["count"]:] == SENT_I32).all(), (what, "rows of tent at or beyond the count are not written")


_DEVICE = {}


def _scene_on_device(key, sc):
    if key not in _DEVICE:
        _DEVICE[key] = (dev_of(sc["d1"]), dev_of(sc["d2"]), dev_of(sc["l2"]))
    return _DEVICE[key]


def _run_scene(key, sc, radii, mutuals=(False, True), chunks=CHUNKS):
    M = rf.scene_distance(key, sc)
    d1, d2, l2 = _scene_on_device(key, sc)
    out = {}
    for r in radii:
        for mutual in mutuals:
            want = rf.ratio_from(M, sc["l2"], r, THR, mutual=mutual)
            for nc in chunks:
                got = raw_ratio(d1, d2, l2, r, mutual=mutual, n_chunks=nc)
                check_against_mirror(got, want, d1.size(0), (key, r, mutual, nc))
            out[(r, mutual)] = want
    return out


# ---- 1, 2: bytes against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", mf.MATRIX_SHAPES)
def test_bytes_against_the_mirror(n1, n2):
    """Partial wave, partial tile, a chunk that starts behind n2, one column; every radius, mutual off and on, five chunk counts."""
    _run_scene(("planted", n1, n2), rf.planted_scene(n1, n2), RADII)


def test_without_frames_and_with_a_distance_cap():
    n1, n2 = 65, 200
    sc = rf.planted_scene(n1, n2)
    M = rf.scene_distance(("planted", n1, n2), sc)
    d1, d2, l2 = _scene_on_device(("planted", n1, n2), sc)
    check_against_mirror(raw_ratio(d1, d2, None, -1.0), rf.ratio_from(M, None, -1.0, THR), n1, "NULL frames without a radius")
    check_against_mirror(raw_ratio(d1, d2, None, -INF), rf.ratio_from(M, None, -1.0, THR), n1, "radius -inf")
    for r in RADII:
        for md in (0.5, 0.0, INF):
            check_against_mirror(raw_ratio(d1, d2, l2, r, max_dist=md, mutual=True), rf.ratio_from(M, sc["l2"], r, THR, md, True), n1, (r, md))
        check_against_mirror(raw_ratio(d1, d2, l2, r, thr=0.95), rf.ratio_from(M, sc["l2"], r, 0.95), n1, (r, 0.95))


@pytest.mark.parametrize("n1,n2", [(1023, 200), (1024, 200), (1025, 200), (2049, 200)])
def test_selection_rounds(n1, n2):
    """One below, at and above one round of the 1024-thread selection, and more than two."""
    want = _run_scene(("planted", n1, n2), rf.planted_scene(n1, n2), RADII, chunks=(0, 3))
    assert 0 < want[(10.0, True)]["count"] < want[(10.0, False)]["count"] < n1
    if n1 > 1024:
        assert want[(-1.0, False)]["keep"][1024] and not want[(-1.0, False)]["keep"][1023]


# ---- 3: against the device code the project already has --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(17, 33), (65, 200), (200, 415)])
def test_against_knn_and_the_distance_matrix(n1, n2):
    import affnet_amd
    from affnet_amd.Losses import distance_matrix_vector
    sc = rf.planted_scene(n1, n2)
    d1, d2, l2 = _scene_on_device(("planted", n1, n2), sc)
    k1d, k1i = (t.cpu().numpy() for t in affnet_amd.knn(d1, d2, 1))
    k2d, k2i = (t.cpu().numpy() for t in affnet_amd.knn(d1, d2, 2))
    M = distance_matrix_vector(d1, d2).cpu().numpy()
    for r in RADII:
        for nc in (0, 2):
            got = raw_ratio(d1, d2, l2, r, n_chunks=nc)
            assert same(got["dist"][:, :1], k1d) and same(got["idx"][:, :1], k1i), (r, nc)
            if r < 0:
                assert same(got["dist"], k2d) and same(got["idx"], k2i), nc
            for s in (0, 1):
                filled = got["idx"][:, s] >= 0
                rows = np.nonzero(filled)[0]
                assert same(got["dist"][rows, s], M[rows, got["idx"][rows, s]]), (r, nc, s)
                assert np.isinf(got["dist"][~filled, s]).all()


# ---- 4: the special scenes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rf.SPECIAL))
def test_special_scenes(name):
    sc = rf.SPECIAL[name]()
    want = _run_scene(name, sc, RADII, chunks=(0, 1, 2))
    if name == "twin":
        d1, d2, l2 = _scene_on_device(name, sc)
        fginn, plain = raw_ratio(d1, d2, l2, 10.0), raw_ratio(d1, d2, l2, -1.0)
        rows_f, rows_p = set(fginn["tent"][:fginn["count"], 0].tolist()), set(plain["tent"][:plain["count"], 0].tolist())
        assert set(sc["planted"].tolist()) <= rows_f and not (set(sc["planted"].tolist()) & rows_p)
    if name == "nine":
        assert want[(10.0, False)]["idx"][0, 1] == 45
    if name == "nan":
        assert np.isnan(want[(10.0, False)]["dist"][1, 0]) and not want[(10.0, False)]["keep"][1]


def test_empty_sides():
    d = dev_of(mf.planted(17, 33)[0])
    l = dev_of(rf.frames(np.zeros((17, 2))))
    e, el = torch.zeros(0, 128, device=DEV), torch.zeros(0, 2, 3, device=DEV)
    for r in RADII:
        for mutual in (False, True):
            got = raw_ratio(d, e, el, r, mutual=mutual)
            assert got["count"] == 0 and (got["idx"] == -1).all() and np.isinf(got["dist"]).all() and (got["tent"] == SENT_I32).all()
            got = raw_ratio(e, d, l, r, mutual=mutual)
            assert got["count"] == 0


# ---- 5: many pairs ---------------------------------------------------------------------------------------------------------------------------
def _many_inputs():
    """Images of 17, 65, 0, 200 and 130 rows on side 1 and 33, 200, 0, 415 and 1 on side 2, from the planted scenes, back to back."""
    shapes = [(17, 33), (65, 200), (200, 415), (130, 1)]
    scs = [rf.planted_scene(a, b) for a, b in shapes]
    D1 = np.concatenate([s["d1"] for s in scs[:2]] + [np.zeros((0, 128), np.float32)] + [s["d1"] for s in scs[2:]])
    D2 = np.concatenate([s["d2"] for s in scs[:2]] + [np.zeros((0, 128), np.float32)] + [s["d2"] for s in scs[2:]])
    L2 = np.concatenate([s["l2"] for s in scs[:2]] + [np.zeros((0, 2, 3), np.float32)] + [s["l2"] for s in scs[2:]])
    c1, c2 = [17, 65, 0, 200, 130], [33, 200, 0, 415, 1]
    return dev_of(D1), dev_of(D2), dev_of(L2), c1, c2


@pytest.mark.parametrize("P", [1, 5])
def test_many_pairs_equal_the_single_pair_calls(P):
    from affnet_amd import ReprojectionStuff as RS
    D1, D2, L2, c1, c2 = _many_inputs()
    o1, o2 = np.concatenate([[0], np.cumsum(c1)]), np.concatenate([[0], np.cumsum(c2)])
    # (image of side 1, image of side 2): an uneven pair, an empty n1, an empty n2, a pair listed twice, and (P = 5) a row out of range
    pairs = [(1, 3)] if P == 1 else [(1, 3), (2, 1), (0, 2), (1, 3), (3, 0)]
    table, n1_max, n2_max = RS.pair_table(c1, c2, pairs)
    if P == 5:
        table[4] = (o1[3], 200, o2[4], 2)            # side 2 ends one row behind o2[4]: two rows from there are one too many
    for r in RADII:
        for mutual in (False, True):
            first = None
            for nc in (0, 3):
                got = raw_ratio_many(D1, D2, L2, table, n1_max, n2_max, r, mutual=mutual, n_chunks=nc)
                if first is None:
                    first = got
                assert all(same(got[k], first[k]) for k in got), "the chunk count changes nothing"
            for p, (a, b) in enumerate(pairs):
                what = (P, r, mutual, p)
                if P == 5 and p == 4:
                    assert first["count"][p] == 0 and (first["idx"][p] == SENT_I32).all() and (first["tent"][p] == SENT_I32).all(), what
                    continue
                n1 = c1[a]
                one = raw_ratio(D1[o1[a]:o1[a + 1]], D2[o2[b]:o2[b + 1]], L2[o2[b]:o2[b + 1]], r, mutual=mutual)
                assert first["count"][p] == one["count"], what
                assert same(first["dist"][p, :n1], one["dist"]) and same(first["idx"][p, :n1], one["idx"]), what
                assert same(first["tent"][p, :one["count"]], one["tent"][:one["count"]]), what
                assert (first["tent"][p, one["count"]:] == SENT_I32).all() and (first["idx"][p, n1:] == SENT_I32).all(), what
                assert (first["dist"][p, n1:] == np.float32(SENT_F32)).all(), what
    got = raw_ratio_many(D1, D2, None, table, n1_max, n2_max, -1.0)
    want = raw_ratio_many(D1, D2, L2, table, n1_max, n2_max, -1.0)
    assert all(same(got[k], want[k]) for k in got), "no frames are read without a radius"


# ---- 6: the chains ---------------------------------------------------------------------------------------------------------------------------
def _same_result(got, want):
    t1, t2, H, inl, info = got
    w1, w2, wH, winl, winfo = want
    assert torch.equal(t1, w1) and torch.equal(t2, w2) and t1.dtype == torch.int64
    assert torch.equal(H, wH) and H.dtype == torch.float64 and H.shape == (3, 3)
    assert torch.equal(inl, winl) and inl.dtype == torch.bool
    assert torch.equal(info["counts"], winfo["counts"])
    assert {k: v for k, v in info.items() if k != "counts"} == {k: v for k, v in winfo.items() if k != "counts"}


def _chain_scene(T, seed, kind):
    sc = gf.repeated_scene(T, seed, kind)
    return tuple(dev_of(sc[k]) for k in ("d1", "d2", "l1", "l2"))


@pytest.mark.parametrize("model,kind", [("homography", gf.PLANAR), ("fundamental", gf.EPIPOLAR)])
def test_chain_is_match_then_verify(model, kind):
    from affnet_amd import ReprojectionStuff as RS
    d1, d2, l1, l2 = _chain_scene(130, 3, kind)
    kw = dict(rounds=4, seed=3) if model == "fundamental" else {}
    for matcher, radius, mutual in (("fginn", 10.0, False), ("fginn", 4.0, True), ("snn", None, False), ("snn", None, True)):
        got = RS.match_and_verify(d1, d2, l1, l2, THR, 3.0, model, 3, matcher=matcher, fginn_radius=10.0 if radius is None else radius, mutual=mutual, **kw)
        t1, t2, dist, idx = RS.match_ratio(d1, d2, l2, radius, THR, mutual=mutual)
        assert torch.equal(got[0], t1) and torch.equal(got[1], t2) and t1.numel() > 0
        H, inl, info = RS.verify_matches(l1, l2, t1, t2, 3.0, model, 3, **kw)
        _same_result(got, (t1, t2, H, inl, info))
    f1, f2, _, _ = RS.match_fginn(d1, d2, l2)
    r1, r2, _, _ = RS.match_ratio(d1, d2, l2, 10.0)
    assert torch.equal(f1, r1) and torch.equal(f2, r2)
    # the default is the reference matcher: the keyword changes no byte
    _same_result(RS.match_and_verify(d1, d2, l1, l2, THR, 3.0, model, 3, matcher="reference", **kw), RS.match_and_verify(d1, d2, l1, l2, THR, 3.0, model, 3, **kw))
    s1, s2, _, _ = RS.match_snn(d1, d2, THR)
    ref = RS.match_and_verify(d1, d2, l1, l2, THR, 3.0, model, 3, **kw)
    assert torch.equal(ref[0], s1) and torch.equal(ref[1], s2)


def test_many_chain_equals_the_loop_of_single_pair_chains():
    import affnet_amd
    from affnet_amd import ReprojectionStuff as RS
    descs, lafs, pairs = [], [], []
    for T, seed in ((130, 3), (65, 4), (17, 5)):
        d1, d2, l1, l2 = _chain_scene(T, seed, gf.PLANAR)
        pairs.append((len(descs), len(descs) + 1))
        descs += [d1, d2]
        lafs += [l1, l2]
    pairs.append((0, 3))
    for model in ("homography", "fundamental"):
        kw = dict(rounds=4, seed=3) if model == "fundamental" else {}
        for matcher, mutual in (("fginn", False), ("fginn", True), ("snn", True), ("reference", False)):
            got = RS.match_and_verify_many(descs, lafs, pairs, THR, 3.0, model, 3, matcher=matcher, mutual=mutual, **kw)
            assert len(got) == len(pairs)
            for (a, b), g in zip(pairs, got):
                _same_result(g, RS.match_and_verify(descs[a], descs[b], lafs[a], lafs[b], THR, 3.0, model, 3, matcher=matcher, mutual=mutual, **kw))
        for g, w in zip(RS.match_and_verify_many(descs, lafs, pairs, THR, 3.0, model, 3, matcher="reference", **kw),
                        RS.match_and_verify_many(descs, lafs, pairs, THR, 3.0, model, 3, **kw)):
            _same_result(g, w)
    # re-ranking and retrieval pass the matcher through
    order, num = RS.spatial_rerank(descs, lafs, 0, [3, 1], matcher="fginn", mutual=True)
    each = {s: RS.match_and_verify(descs[0], descs[s], lafs[0], lafs[s], matcher="fginn", mutual=True)[4]["num_inliers"] for s in (3, 1)}
    assert order == [1, 3] and num == [each[1], each[3]] and num[0] > num[1]
    assert RS.spatial_rerank(descs, lafs, 0, [3, 1], matcher="reference") == RS.spatial_rerank(descs, lafs, 0, [3, 1])
    index = affnet_amd.DescriptorIndex(descs, lafs)
    for entry in index.retrieve(descs[0], lafs[0], top=3, exclude=0, matcher="fginn"):
        t1, t2, H, inl, info = RS.match_and_verify(descs[0], descs[entry["image"]], lafs[0], lafs[entry["image"]], matcher="fginn")
        assert torch.equal(entry["tent_in_1"], t1) and torch.equal(entry["tent_in_2"], t2) and torch.equal(entry["H"], H)
        assert torch.equal(entry["inliers"], inl) and entry["num_inliers"] == info["num_inliers"]


# ---- 7: argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_library_usable():
    from affnet_amd import _lib
    lib, ptr, check, ctx, st, dev = _api()
    n1, n2 = 65, 200
    sc = rf.planted_scene(n1, n2)
    d1, d2, l2 = _scene_on_device(("planted", n1, n2), sc)
    want = rf.ratio_from(rf.scene_distance(("planted", n1, n2), sc), sc["l2"], 10.0, THR, mutual=True)
    dist, idx = full((n1, 2), SENT_F32, torch.float32), full((n1, 2), SENT_I32, torch.int32)
    tent, cnt = full((n1, 2), SENT_I32, torch.int32), full((1,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_match_ratio_scratch_bytes(n1, n2, 0) + 16, dtype=torch.uint8, device=dev)
    pairs = torch.tensor([[0, n1, 0, n2]], dtype=torch.int32, device=dev)
    ok = dict(d1=d1, n1=n1, d2=d2, n2=n2, dim=128, l2=l2, r=10.0, md=INF, flags=1, nc=0, dist=dist, idx=idx, tent=tent, count=cnt, pairs=pairs, P=1, off=0)
    nan = float("nan")
    bad = [dict(d1=None), dict(d2=None), dict(l2=None), dict(l2=None, r=0.0), dict(dist=None), dict(idx=None), dict(tent=None), dict(count=None), dict(n1=-1),
           dict(n2=-1), dict(dim=64), dict(flags=2), dict(r=nan), dict(r=INF), dict(md=nan), dict(nc=-1), dict(nc=65536), dict(off=4)]

    def call(many, **kw):
        a = dict(ok, **kw)
        p = {k: (None if a[k] is None else ptr(a[k])) for k in ("d1", "d2", "l2", "dist", "idx", "tent", "count", "pairs")}
        scr = _lib.C.c_void_p(scratch.data_ptr() + a["off"])
        if many:
            return lib.affnet_match_ratio_many(ctx, p["d1"], n1, p["d2"], n2, a["dim"], p["l2"], p["pairs"], a["P"], a["n1"], a["n2"], a["r"], THR, a["md"],
                                               a["flags"], a["nc"], p["dist"], p["idx"], p["tent"], p["count"], scr, st)
        return lib.affnet_match_ratio(ctx, p["d1"], a["n1"], p["d2"], a["n2"], a["dim"], p["l2"], a["r"], THR, a["md"], a["flags"], a["nc"], p["dist"], p["idx"],
                                      p["tent"], p["count"], scr, st)
    for many in (False, True):
        for kw in bad + ([dict(pairs=None), dict(P=-1), dict(P=65536)] if many else []):
            assert call(many, **kw) == _lib.ERR_INVALID, (many, kw)
        torch.cuda.synchronize()
        assert (dist.cpu().numpy() == np.float32(SENT_F32)).all() and (cnt.cpu().numpy() == SENT_I32).all(), "a refused call writes nothing"
        assert call(many) == _lib.OK
        got = dict(dist=dist.cpu().numpy(), idx=idx.cpu().numpy(), tent=tent.cpu().numpy(), count=int(cnt.item()))
        check_against_mirror(got, want, n1, ("after the refused calls", many))
        for t, v in ((dist, SENT_F32), (idx, SENT_I32), (tent, SENT_I32), (cnt, SENT_I32)):
            t.fill_(v)
    assert call(False, l2=None, r=-1.0) == _lib.OK and call(True, l2=None, r=-1.0) == _lib.OK
    torch.cuda.synchronize()
