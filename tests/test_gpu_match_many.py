"""MI355X: matching and verifying many image pairs in one device call (affnet_match_snn_many, affnet_verify_matches_many,
ReprojectionStuff.match_and_verify_many / spatial_rerank) against the single-pair calls, which the other tests pin to the oracle and to the
float64 restatement.  The batched kernels run the single-pair device functions on each pair's segments, so the tolerance is zero: every
comparison below is on the bytes (which, unlike array_equal, also holds a NaN distance to its bit pattern)."""
import numpy as np
import pytest
import torch

import _spatial_fp64 as sp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TH = 3.0
SENT_F32, SENT_I32, SENT_U8 = -7.5, -7, 0xAB
COUNTS = [1, 15, 16, 17, 63, 64, 65, 130, 200]       # one below, at, one above the 16-column tile and the 64-row workgroup of the row-minimum kernel; > 1 workgroup


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


def raw_snn(d1, d2, thr=0.8):
    """affnet_match_snn on two device tensors -> numpy (md, idx, md2, tent (n1,2) with sentinel rows behind the count, count)."""
    lib, ptr, check, ctx, st, dev = _api()
    n1, n2 = d1.size(0), d2.size(0)
    md, md2, idx = full((n1,), SENT_F32, torch.float32), full((n1,), SENT_F32, torch.float32), full((n1,), SENT_I32, torch.int32)
    tent, cnt = full((n1, 2), SENT_I32, torch.int32), full((1,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=dev)
    check(lib.affnet_match_snn(ctx, ptr(d1), n1, ptr(d2), n2, 128, thr, ptr(md), ptr(idx), ptr(md2), ptr(tent), ptr(cnt), ptr(scratch), st), ctx, "affnet_match_snn")
    return dict(md=md.cpu().numpy(), idx=idx.cpu().numpy(), md2=md2.cpu().numpy(), tent=tent.cpu().numpy(), count=int(cnt.item()))


def raw_snn_many(D1, D2, table, n1_max, n2_max, thr=0.8):
    lib, ptr, check, ctx, st, dev = _api()
    P = table.shape[0]
    md, md2, idx = full((P, n1_max), SENT_F32, torch.float32), full((P, n1_max), SENT_F32, torch.float32), full((P, n1_max), SENT_I32, torch.int32)
    tent, cnt = full((P, n1_max, 2), SENT_I32, torch.int32), full((P,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_match_many_scratch_bytes(P, n1_max, n2_max), dtype=torch.uint8, device=dev)
    pairs = torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev)
    check(lib.affnet_match_snn_many(ctx, ptr(D1), D1.size(0), ptr(D2), D2.size(0), 128, ptr(pairs), P, n1_max, n2_max, thr, ptr(md), ptr(idx), ptr(md2), ptr(tent),
                                    ptr(cnt), ptr(scratch), st), ctx, "affnet_match_snn_many")
    return dict(md=md.cpu().numpy(), idx=idx.cpu().numpy(), md2=md2.cpu().numpy(), tent=tent.cpu().numpy(), count=cnt.cpu().numpy(), d_tent=tent, d_count=cnt)


def raw_verify(l1, l2, tent, model, lo_iters):
    """affnet_verify_matches on device frames and a (T,2) numpy tentative list, all T rows valid -> numpy dict."""
    lib, ptr, check, ctx, st, dev = _api()
    T = tent.shape[0]
    dt = torch.zeros(max(T, 1), 2, dtype=torch.int32, device=dev)
    dt[:T] = torch.from_numpy(np.ascontiguousarray(tent, np.int32)).to(dev)
    counts, inl = full((max(T, 1),), SENT_I32, torch.int32), full((max(T, 1),), SENT_U8, torch.uint8)
    H, summ = full((9,), float("nan"), torch.float64), full((4,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_verify_scratch_bytes(T), dtype=torch.uint8, device=dev)
    check(lib.affnet_verify_matches(ctx, ptr(l1), l1.size(0), ptr(l2), l2.size(0), ptr(dt), None, T, TH, model, lo_iters, ptr(counts), ptr(H), ptr(inl), ptr(summ),
                                    ptr(scratch), st), ctx, "affnet_verify_matches")
    return dict(counts=counts.cpu().numpy()[:T], inlier=inl.cpu().numpy()[:T], H=H.cpu().numpy(), summary=summ.cpu().numpy())


def raw_verify_many(L1, L2, table, d_tent, d_count, t_max, model, lo_iters):
    lib, ptr, check, ctx, st, dev = _api()
    P = table.shape[0]
    counts, inl = full((P, max(t_max, 1)), SENT_I32, torch.int32), full((P, max(t_max, 1)), SENT_U8, torch.uint8)
    H, summ = full((P, 9), float("nan"), torch.float64), full((P, 4), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_verify_many_scratch_bytes(P, t_max), dtype=torch.uint8, device=dev)
    pairs = torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev)
    check(lib.affnet_verify_matches_many(ctx, ptr(L1), L1.size(0), ptr(L2), L2.size(0), ptr(pairs), P, ptr(d_tent), ptr(d_count), t_max, TH, model, lo_iters,
                                         ptr(counts), ptr(H), ptr(inl), ptr(summ), ptr(scratch), st), ctx, "affnet_verify_matches_many")
    return dict(counts=counts.cpu().numpy(), inlier=inl.cpu().numpy(), H=H.cpu().numpy(), summary=summ.cpu().numpy())


_SET = {}


def image_set():
    """The ragged image set, computed once and never modified: unit descriptors (noisy copies of rows of one pool of 200 unit vectors, in a random
    order per image, so that every pair has matches that pass the ratio test and matches that do not), random frames, the device buffers."""
    if not _SET:
        from affnet_amd import ReprojectionStuff as RS
        rng = np.random.default_rng(11)
        pool = rng.normal(size=(200, 128))
        descs, lafs = [], []
        for n in COUNTS:
            d = pool[rng.permutation(200)[:n]] + 0.06 * rng.normal(size=(n, 128))
            descs.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
            lafs.append(sp.random_frames(rng, n).astype(np.float32))
        off = np.concatenate([[0], np.cumsum(COUNTS)])
        _SET.update(descs=descs, lafs=lafs, off=off, RS=RS, D=torch.from_numpy(np.concatenate(descs)).to(DEV), L=torch.from_numpy(np.concatenate(lafs)).to(DEV))
    return _SET


@pytest.fixture(scope="module", autouse=True)
def recorded_single_pair_calls():
    """Outputs of the single-pair entry points, recorded before the first batched call of this process (this module makes the only ones, and
    this fixture runs in front of its first test)."""
    s = image_set()
    a, b = s["D"][s["off"][7]:s["off"][8]], s["D"][s["off"][8]:s["off"][9]]
    la, lb = s["L"][s["off"][7]:s["off"][8]], s["L"][s["off"][8]:s["off"][9]]
    m = raw_snn(a, b)
    v = raw_verify(la, lb, m["tent"][:m["count"]], sp.HOMOGRAPHY, 3)
    return dict(a=a, b=b, la=la, lb=lb, m=m, v=v)


def test_matcher_equals_the_loop():
    s = image_set()
    n = len(COUNTS)
    pairs = [(i, j) for i in range(n) for j in range(n)]        # every (n1, n2) edge combination; (i, i) are self-pairs, every image is a query 9 times
    table, n1_max, n2_max = s["RS"].pair_table(COUNTS, COUNTS, pairs)
    assert (n1_max, n2_max) == (200, 200)
    got = raw_snn_many(s["D"], s["D"], table, n1_max, n2_max)
    seen = set()
    for p, (i, j) in enumerate(pairs):
        n1 = COUNTS[i]
        want = raw_snn(s["D"][s["off"][i]:s["off"][i + 1]], s["D"][s["off"][j]:s["off"][j + 1]])
        k = want["count"]
        assert got["count"][p] == k, (i, j)
        for name in ("md", "idx", "md2"):
            assert same(got[name][p, :n1], want[name]), (name, i, j)
        assert same(got["tent"][p, :k], want["tent"][:k]), (i, j)
        assert (got["tent"][p, k:] == SENT_I32).all() and (want["tent"][k:] == SENT_I32).all(), "rows at or beyond the count are not written"
        assert (got["md"][p, n1:] == SENT_F32).all() and (got["md2"][p, n1:] == SENT_F32).all() and (got["idx"][p, n1:] == SENT_I32).all(), "rows n1 .. n1_max"
        assert got["idx"][p, :n1].min() >= 0 and got["idx"][p, :n1].max() < COUNTS[j], "indices are local to the pair's segments"
        seen.add(0 if k == 0 else (1 if k == n1 else 2))
    assert seen == {0, 1, 2} or seen == {1, 2}, "the ratio test passes some rows and refuses others"
    again = raw_snn_many(s["D"], s["D"], table, n1_max, n2_max)
    assert all(same(again[k], got[k]) for k in ("md", "idx", "md2", "tent", "count"))


_PLANTED_T = [(1, 3), (2, 4), (127, 5), (128, 6), (129, 7), (257, 8)]       # (T, seed): the tile and chunk edges of the scoring kernel (128)


@pytest.mark.parametrize("model,lo_iters", [(sp.HOMOGRAPHY, 3), (sp.AFFINE, 3), (sp.HOMOGRAPHY, 0), (sp.AFFINE, 0)])
def test_verification_equals_the_loop(model, lo_iters):
    cases = [sp.planted(T, seed) for T, seed in _PLANTED_T]
    Ts = [T for T, _ in _PLANTED_T]
    t_max = max(Ts)
    L1 = torch.from_numpy(np.concatenate([c[0] for c in cases])).to(DEV)
    L2 = torch.from_numpy(np.concatenate([c[1] for c in cases])).to(DEV)
    off = np.concatenate([[0], np.cumsum(Ts)])
    table = np.array([[off[p], Ts[p], off[p], Ts[p]] for p in range(len(Ts))], np.int32)
    tent = np.full((len(Ts), t_max, 2), 1 << 20, np.int32)          # rows behind a pair's count: an index far outside, never read
    for p, c in enumerate(cases):
        tent[p, :Ts[p]] = c[2]
    d_tent, d_count = torch.from_numpy(tent).to(DEV), torch.tensor(Ts, dtype=torch.int32, device=DEV)
    got = raw_verify_many(L1, L2, table, d_tent, d_count, t_max, model, lo_iters)
    for p, c in enumerate(cases):
        T = Ts[p]
        want = raw_verify(torch.from_numpy(c[0]).to(DEV), torch.from_numpy(c[1]).to(DEV), c[2], model, lo_iters)
        assert same(got["counts"][p, :T], want["counts"]) and same(got["inlier"][p, :T], want["inlier"]), T
        assert same(got["summary"][p], want["summary"]) and same(got["H"][p], want["H"]), (T, got["summary"][p], want["summary"])
        assert (got["counts"][p, T:] == SENT_I32).all() and (got["inlier"][p, T:] == SENT_U8).all(), "rows at or beyond the count are not written"
    assert got["summary"][:, 3].tolist().count(0) >= 3, "the larger planted cases are verified without a flag"
    again = raw_verify_many(L1, L2, table, d_tent, d_count, t_max, model, lo_iters)
    assert all(same(again[k], got[k]) for k in got), "same bytes every run"


def _planted_pair(T, seed, rng):
    """The construction of test_gpu_spatial.test_match_and_verify_is_match_then_verify_bit_for_bit: planted frames, and descriptors that match
    along the planted rows."""
    l1, l2, tent, planted = sp.planted(T, seed)
    d1 = rng.normal(size=(T, 128))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 = rng.normal(size=(T, 128))
    src = np.nonzero(planted)[0]
    d2[tent[src, 1]] = d1[src] + 0.02 * rng.normal(size=(len(src), 128))
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    return t(d1), t(l1), t(d2), t(l2), len(src)


def _same_result(got, want):
    t1, t2, H, inl, info = got
    w1, w2, wH, winl, winfo = want
    assert torch.equal(t1, w1) and torch.equal(t2, w2) and t1.dtype == torch.int64
    assert torch.equal(H, wH) and H.dtype == torch.float64 and H.shape == (3, 3)
    assert torch.equal(inl, winl) and inl.dtype == torch.bool
    assert torch.equal(info["counts"], winfo["counts"])
    assert {k: v for k, v in info.items() if k != "counts"} == {k: v for k, v in winfo.items() if k != "counts"}


def test_chain_and_rerank():
    from affnet_amd import ReprojectionStuff as RS
    rng = np.random.default_rng(5)
    descs, lafs, pairs, planted = [], [], [], []
    for T, seed in ((300, 1), (129, 2), (64, 3), (1, 4)):
        d1, l1, d2, l2, n_pl = _planted_pair(T, seed, rng)
        pairs.append((len(descs), len(descs) + 1))
        descs += [d1, d2]
        lafs += [l1, l2]
        planted.append(n_pl)
    # image 8: 300 independently random frames and descriptors
    d = rng.normal(size=(300, 128))
    descs.append(torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).to(DEV))
    lafs.append(torch.from_numpy(sp.random_frames(rng, 300).astype(np.float32)).to(DEV))
    for model in ("homography", "affine"):
        got = RS.match_and_verify_many(descs, lafs, pairs, 0.8, TH, model, 3)
        assert len(got) == 4
        for (a, b), g in zip(pairs, got):
            _same_result(g, RS.match_and_verify(descs[a], descs[b], lafs[a], lafs[b], 0.8, TH, model, 3))
        if model == "homography":
            assert got[0][4]["flags"] == 0 and got[0][4]["num_inliers"] >= planted[0] >= 100
    # re-ranking: the planted partner of image 0 (about half its rows are planted inliers) against the random image, random image first in the shortlist
    order, num = RS.spatial_rerank(descs, lafs, 0, [8, 1])
    assert order == [1, 8] and num[0] >= planted[0] > num[1]
    each = {s: RS.match_and_verify(descs[0], descs[s], lafs[0], lafs[s])[4]["num_inliers"] for s in (8, 1)}
    assert num == [each[1], each[8]]
    assert RS.spatial_rerank(descs, lafs, 0, []) == ([], [])


def test_table_guard():
    """Ordinary argument validation, seen through what the call returns: a row of the table that is out of range is tested before anything is
    loaded or stored through it."""
    s = image_set()
    off, rows = s["off"], int(s["off"][-1])
    n1_max, n2_max = 65, 130
    i3, i6, i7, i8 = int(off[3]), int(off[6]), int(off[7]), int(off[8])
    big = 0x7fffffff
    table = np.array([[i3, 17, i7, 130],            # 0 valid
                      [-1, 17, i7, 130],            # 1 negative row1
                      [i3, 17, i7, -130],           # 2 negative n2
                      [rows - 3, 17, i7, 130],      # 3 row1 + n1 > rows1
                      [i3, 17, rows - 3, 130],      # 4 row2 + n2 > rows2
                      [i7, 130, i3, 17],            # 5 n1 > n1_max
                      [i3, 17, i7, 0],              # 6 empty side 2
                      [i3, 0, i7, 130],             # 7 empty side 1
                      [big, big, i7, 130],          # 8 row1 + n1 beyond int32
                      [i6, 65, i3, 17],             # 9 valid, n1 at the cap
                      [i3, 17, i8, 200]], np.int32)  # 10 n2 > n2_max
    bad, empty, valid = [1, 2, 3, 4, 5, 8], [6, 7], [0, 9]
    m = raw_snn_many(s["D"], s["D"], table, n1_max, n2_max)
    v = raw_verify_many(s["L"], s["L"], table, m["d_tent"], m["d_count"], n1_max, sp.HOMOGRAPHY, 3)
    for p in bad + empty + [10]:
        assert m["count"][p] == 0, p
        assert (m["md"][p] == SENT_F32).all() and (m["md2"][p] == SENT_F32).all() and (m["idx"][p] == SENT_I32).all() and (m["tent"][p] == SENT_I32).all(), p
        assert (v["counts"][p] == SENT_I32).all() and (v["inlier"][p] == SENT_U8).all(), p
        assert np.array_equal(v["H"][p].reshape(3, 3), np.eye(3)), p
    for p in bad:
        assert v["summary"][p].tolist() == [-1, 0, 0, 9], (p, v["summary"][p])
    for p in empty + [10]:      # (the verification has no cap on n2: a row that only the matcher's n2_max refuses is an empty list to it)
        assert v["summary"][p].tolist() == [-1, 0, 0, 1], (p, v["summary"][p])
    for p in valid:
        r1, n1, r2, n2 = table[p].tolist()
        want = raw_snn(s["D"][r1:r1 + n1], s["D"][r2:r2 + n2])
        k = want["count"]
        assert m["count"][p] == k > 0 and same(m["md"][p, :n1], want["md"]) and same(m["idx"][p, :n1], want["idx"]) and same(m["md2"][p, :n1], want["md2"])
        assert same(m["tent"][p, :k], want["tent"][:k]) and (m["tent"][p, k:] == SENT_I32).all()
        wv = raw_verify(s["L"][r1:r1 + n1], s["L"][r2:r2 + n2], want["tent"][:k], sp.HOMOGRAPHY, 3)
        assert same(v["counts"][p, :k], wv["counts"]) and same(v["inlier"][p, :k], wv["inlier"]) and same(v["summary"][p], wv["summary"]) and same(v["H"][p], wv["H"])
        assert (v["counts"][p, k:] == SENT_I32).all() and (v["inlier"][p, k:] == SENT_U8).all()


def test_boundary(recorded_single_pair_calls):
    lib, ptr, check, ctx, st, dev = _api()
    from affnet_amd import _lib
    s = image_set()
    table, n1_max, n2_max = s["RS"].pair_table(COUNTS, COUNTS, [(7, 8), (8, 7)])
    # no pair: OK, nothing is written
    buf = full((64,), SENT_I32, torch.int32)
    pairs = torch.from_numpy(table).to(dev)
    args = lambda **kw: dict(dict(dim=128, pairs=ptr(pairs), P=0, n1=n1_max), **kw)

    def snn(**kw):
        a = args(**kw)
        return lib.affnet_match_snn_many(ctx, ptr(s["D"]), s["D"].size(0), ptr(s["D"]), s["D"].size(0), a["dim"], a["pairs"], a["P"], a["n1"], n2_max, 0.8, ptr(buf),
                                         ptr(buf), ptr(buf), ptr(buf), ptr(buf), ptr(buf), st)
    assert snn() == _lib.OK
    assert lib.affnet_verify_matches_many(ctx, ptr(s["L"]), s["L"].size(0), ptr(s["L"]), s["L"].size(0), ptr(pairs), 0, ptr(buf), ptr(buf), 16, TH, 1, 3, ptr(buf),
                                          ptr(buf), ptr(buf), ptr(buf), ptr(buf), st) == _lib.OK
    torch.cuda.synchronize()
    assert (buf == SENT_I32).all()
    for kw in (dict(dim=64, P=2), dict(pairs=None, P=2), dict(n1=-1, P=2)):
        assert snn(**kw) == _lib.ERR_INVALID, kw
        assert b"match_snn_many" in lib.affnet_last_error(ctx), kw
    assert lib.affnet_verify_matches_many(ctx, ptr(s["L"]), s["L"].size(0), ptr(s["L"]), s["L"].size(0), None, 2, ptr(buf), ptr(buf), 16, TH, 1, 3, ptr(buf), ptr(buf),
                                          ptr(buf), ptr(buf), ptr(buf), st) == _lib.ERR_INVALID
    assert b"verify_matches_many" in lib.affnet_last_error(ctx)
    assert lib.affnet_verify_matches_many(ctx, ptr(s["L"]), s["L"].size(0), ptr(s["L"]), s["L"].size(0), ptr(pairs), 2, ptr(buf), ptr(buf), -1, TH, 1, 3, ptr(buf),
                                          ptr(buf), ptr(buf), ptr(buf), ptr(buf), st) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert (buf == SENT_I32).all(), "a refused call writes nothing"
    # the single-pair entry points after batched calls (here, and in the tests in front of this one): the bytes recorded before the first batched call
    r = recorded_single_pair_calls
    got = raw_snn_many(s["D"], s["D"], table, n1_max, n2_max)
    m = raw_snn(r["a"], r["b"])
    assert m["count"] == r["m"]["count"] == got["count"][0] and all(same(m[k], r["m"][k]) for k in ("md", "idx", "md2", "tent"))
    v = raw_verify(r["la"], r["lb"], m["tent"][:m["count"]], sp.HOMOGRAPHY, 3)
    assert all(same(v[k], r["v"][k]) for k in v)
