"""MI355X: the int8 descriptor index (csrc/knn_q8.hip affnet_quantize_desc / affnet_knn_q8, affnet_amd/retrieval.py).  The quantiser and the
search against the numpy mirror (tests/_knn_q8.py) on the bytes of every output: the arithmetic is integer and exact, so the tolerance is zero,
for every number of column chunks.  Then the quantised index against the fp32 one on the vote fixture of tests/_knn_fp64.py and on the ragged
image set with frames, down to the batched verification."""
import numpy as np
import pytest
import torch

import _knn_fp64 as kf
import _knn_q8 as kq
import _spatial_fp64 as sp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_F32, SENT_I32, SENT_I8 = -7.5, -7, -7
NCH = [0, 1, 2, 3, 7, 30]
SCALE = 335.07


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


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def raw_quantize(x, scale):
    """affnet_quantize_desc on a device tensor -> numpy (q (n,128) int8, sq (n,) int32), the outputs pre-filled with sentinels."""
    lib, ptr, check, ctx, st, d = _api()
    n = x.size(0)
    q, sq = full((n + 1, 128), SENT_I8, torch.int8), full((n + 1,), SENT_I32, torch.int32)
    check(lib.affnet_quantize_desc(ctx, ptr(x), n, 128, scale, ptr(q), ptr(sq), st), ctx, "affnet_quantize_desc")
    q, sq = q.cpu().numpy(), sq.cpu().numpy()
    assert (q[n:] == SENT_I8).all() and (sq[n:] == SENT_I32).all(), "rows behind n are not written"
    return q[:n], sq[:n]


def raw_knn(q, db, k, skip=(0, 0), nc=0, scale=SCALE):
    """affnet_knn_q8 on two int8 numpy arrays -> numpy (dist2, dist, idx), (n1,k) each, the outputs pre-filled with sentinels."""
    lib, ptr, check, ctx, st, d = _api()
    n1, n2 = q.shape[0], db.shape[0]
    one = torch.zeros(16, dtype=torch.int32, device=d)          # stands in for empty inputs: never read, but the boundary refuses NULL
    dq, dqs = (dev(q), dev(kq.sq(q))) if n1 else (one, one)
    ddb, ddbs = (dev(db), dev(kq.sq(db))) if n2 else (one, one)
    d2, dist, idx = full((n1 + 1, k), SENT_I32, torch.int32), full((n1 + 1, k), SENT_F32, torch.float32), full((n1 + 1, k), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_knn_q8_scratch_bytes(n1, n2, k, nc), dtype=torch.uint8, device=d)
    check(lib.affnet_knn_q8(ctx, ptr(dq), ptr(dqs), n1, ptr(ddb), ptr(ddbs), n2, 128, k, skip[0], skip[1], nc, scale, ptr(d2), ptr(dist), ptr(idx), ptr(scratch), st),
          ctx, "affnet_knn_q8")
    d2, dist, idx = d2.cpu().numpy(), dist.cpu().numpy(), idx.cpu().numpy()
    assert (d2[n1:] == SENT_I32).all() and (dist[n1:] == SENT_F32).all() and (idx[n1:] == SENT_I32).all(), "rows behind n1 are not written"
    return d2[:n1], dist[:n1], idx[:n1]


def check_all_chunks(q, db, k, skip=(0, 0), scale=SCALE, ncs=NCH):
    want = kq.expected(kq.dist2(q, db), k, scale, skip)
    for nc in ncs:
        got = raw_knn(q, db, k, skip, nc, scale)
        assert same(got[2], want[2]), (nc, np.argwhere(got[2] != want[2])[:4])
        assert same(got[0], want[0]) and same(got[1], want[1]), nc
    return want


# ---- quantiser ----

def quantiser_input(n, scale):
    """Values whose products with `scale` reach past +-127 on both sides; row 0: four values that clip, then exact halves at scale 2
    (x = ..., -0.25, 0.25, 0.75, 1.25, ...: x * scale = -59.5, ..., 63.5), row 1: NaN, +-inf and huge numbers, row 2: zeros."""
    rng = np.random.default_rng(50 + n)
    x = (rng.uniform(-140.0, 140.0, size=(n, 128)) / scale).astype(np.float32)
    x[0] = ((np.arange(128) - 63.5) / scale).astype(np.float32)
    x[0, :4] = (np.array([-200.0, 200.0, -127.5, 127.5]) / scale).astype(np.float32)
    if n > 1:
        x[1, 0::7], x[1, 1::7], x[1, 2::7], x[1, 3::7], x[1, 4::7] = np.nan, np.inf, -np.inf, 1e30, -1e30
    if n > 2:
        x[2] = 0.0
    return x


@pytest.mark.parametrize("scale", [2.0, SCALE])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_quantiser_against_the_mirror(n, scale):
    x = quantiser_input(n, scale)
    want_q, want_sq = kq.quantize(x, scale)
    q, sq = raw_quantize(dev(x), scale)
    assert same(q, want_q), np.argwhere(q != want_q)[:4]
    assert same(sq, want_sq) and (sq.astype(np.int64) == (q.astype(np.int64) ** 2).sum(1)).all()
    if scale == 2.0:          # the products are exact: halves go to the even neighbour
        assert x[0, 63:67].tolist() == [-0.25, 0.25, 0.75, 1.25]
        assert q[0, 4:].tolist() == [int(np.rint(i - 63.5)) for i in range(4, 128)] and q[0, :4].tolist() == [-127, 127, -127, 127]
        assert q[0, 60:68].tolist() == [-4, -2, -2, 0, 0, 2, 2, 4]
    assert (q == 127).any() and (q == -127).any() and not (q == -128).any(), "values clip on both sides"
    if n > 1:
        assert q[1, :5].tolist() == [0, 127, -127, 127, -127]
    if n > 2:
        assert not q[2].any() and sq[2] == 0


def test_quantiser_python_layer():
    from affnet_amd import retrieval as R
    x = quantiser_input(65, SCALE)
    q, sq = R.quantize(dev(x), SCALE)
    want_q, want_sq = kq.quantize(x, np.float32(SCALE))
    assert q.dtype == torch.int8 and sq.dtype == torch.int32 and same(q.cpu().numpy(), want_q) and same(sq.cpu().numpy(), want_sq)
    q, sq = R.quantize(torch.zeros(0, 128, device=DEV), SCALE)
    assert q.shape == (0, 128) and sq.shape == (0,)
    v = kf.vote_setup()
    assert R.quantization_scale([dev(d) for d in v["descs"]]) == float(np.float32(127.0 / float(np.abs(v["D"]).max())))
    # n = 0 is a no-op at the boundary
    lib, ptr, check, ctx, st, d = _api()
    buf = full((64,), SENT_I32, torch.int32)
    assert lib.affnet_quantize_desc(ctx, ptr(buf), 0, 128, 2.0, ptr(buf), ptr(buf), st) == 0
    torch.cuda.synchronize()
    assert (buf == SENT_I32).all()


# ---- search ----

# every n1 (with the row blocks 128 of k > 2 and 256 of k <= 2, each - 1, + 1), n2 and k of the issue appears, and each case runs with every n_chunks
CASES = [(1, 1, 1), (15, 15, 2), (16, 16, 3), (17, 17, 4), (63, 79, 5), (64, 80, 6), (65, 81, 7), (130, 1000, 8), (127, 1000, 3), (128, 81, 8),
         (129, 1000, 5), (255, 1000, 1), (256, 79, 2), (257, 1000, 2), (257, 1000, 1), (129, 17, 4), (1, 1000, 8), (130, 1, 8), (64, 16, 1), (17, 80, 2),
         (65, 15, 6), (16, 1000, 7), (256, 1000, 4), (63, 1000, 2)]


@pytest.mark.parametrize("n1,n2,k", CASES)
def test_search_against_the_mirror(n1, n2, k):
    check_all_chunks(kq.random_rows(n1, 1000 + n1), kq.random_rows(n2, 2000 + n2), k)


def test_ties_go_to_the_lower_row():
    rng = np.random.default_rng(7)
    base = kq.random_rows(40, 3)
    where = rng.permutation(np.repeat(np.arange(40), 3))          # database row -> base row: every base row stored three times, scattered
    db = np.ascontiguousarray(base[where])
    spans = [len(set(np.nonzero(where == b)[0] // 64)) > 1 for b in range(40)]          # n_chunks = 2: the chunks meet at column 64
    assert any(spans), "a wrong fixture: no triple crosses a chunk border"
    q = kq.random_rows(33, 4)
    d2, dist, idx = check_all_chunks(q, db, 8)
    assert (where[idx[:, 0]] == where[idx[:, 1]]).all() and (where[idx[:, 1]] == where[idx[:, 2]]).all(), "the three copies of the nearest row lead"
    assert ((d2[:, :-1] < d2[:, 1:]) | ((d2[:, :-1] == d2[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))).all() and (d2[:, 0] == d2[:, 2]).all()
    # query rows that are database rows: three zeros in front
    d2, dist, idx = check_all_chunks(base[:17], db, 8)
    assert (d2[:, :3] == 0).all() and (dist[:, :3] == 0).all() and (d2[:, 3] > 0).all()


def test_extremes():
    q = np.full((3, 128), 127, np.int8)
    db = np.stack([np.full(128, -127, np.int8), np.full(128, 127, np.int8), np.zeros(128, np.int8)])
    d2, dist, idx = check_all_chunks(q, db, 3, ncs=[0, 1, 2])
    assert idx.tolist() == [[1, 2, 0]] * 3 and d2.tolist() == [[0, 128 * 127 * 127, 8258048]] * 3
    assert dist[0, 0] == 0.0 and dist[0, 2] == np.sqrt(np.float32(8258048)) / np.float32(SCALE)
    d2, dist, idx = check_all_chunks(-q, db, 1, ncs=[0, 1])
    assert idx.tolist() == [[0]] * 3 and d2.tolist() == [[0]] * 3


# n2 = 415, n_chunks = 3: 13 steps of 32 columns, 5 per chunk, so chunk 1 owns columns [160, 320)
SKIPS = [(18, 5),          # inside one tile
         (155, 10),        # straddles two tiles and the border of chunks 0 / 1
         (160, 160),       # a whole chunk
         (0, 415),         # everything
         (100, 0),         # no skip
         (400, 100),       # reaches past n2
         (-5, 10),         # starts in front of 0
         (500, 3)]         # behind n2 altogether


@pytest.mark.parametrize("skip", SKIPS)
def test_skip_range(skip):
    q, db = kq.random_rows(65, 11), kq.random_rows(415, 12)
    for k in (2, 8):
        d2, dist, idx = check_all_chunks(q, db, k, skip)
        lo, hi = max(skip[0], 0), skip[0] + skip[1]
        assert not ((idx >= lo) & (idx < hi)).any()
        if skip == (0, 415):
            assert (idx == -1).all() and np.isposinf(dist).all() and (d2 == kq.INT32_MAX).all()


def test_fewer_candidates_than_k():
    q, db = kq.random_rows(17, 21), kq.random_rows(415, 22)
    d2, dist, idx = check_all_chunks(q, db[:3], 8)
    assert (idx[:, 3:] == -1).all() and np.isposinf(dist[:, 3:]).all() and (d2[:, 3:] == kq.INT32_MAX).all() and (idx[:, :3] >= 0).all()
    d2, dist, idx = check_all_chunks(q, db[:0], 8)
    assert idx.shape == (17, 8) and (idx == -1).all() and np.isposinf(dist).all() and (d2 == kq.INT32_MAX).all()
    d2, dist, idx = check_all_chunks(q, db[:3], 2, (1, 1))          # two candidates left by the skip range
    assert set(idx.ravel().tolist()) == {0, 2}
    d2, dist, idx = check_all_chunks(q, db[:40], 8, (3, 35))          # five left of 40
    assert (idx[:, 5:] == -1).all() and (idx[:, :5] >= 0).all()


def test_no_query_row_and_refused_calls_write_nothing():
    lib, ptr, check, ctx, st, d = _api()
    buf = full((4096,), SENT_I32, torch.int32)
    p = ptr(buf)
    assert lib.affnet_knn_q8(ctx, p, p, 0, p, p, 415, 128, 8, 0, 0, 0, SCALE, p, p, p, p, st) == 0
    for bad in (dict(k=0), dict(k=9), dict(dim=64), dict(nc=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf"))):
        a = dict(dict(k=8, dim=128, nc=0, scale=SCALE), **bad)
        assert lib.affnet_knn_q8(ctx, p, p, 4, p, p, 4, a["dim"], a["k"], 0, 0, a["nc"], a["scale"], p, p, p, p, st) == -1, bad
        assert b"knn_q8" in lib.affnet_last_error(ctx)
        if "dim" in bad or "scale" in bad:
            assert lib.affnet_quantize_desc(ctx, p, 4, a["dim"], a["scale"], p, p, st) == -1, bad
            assert b"quantize_desc" in lib.affnet_last_error(ctx)
    torch.cuda.synchronize()
    assert (buf == SENT_I32).all(), "a refused call writes nothing"
    from affnet_amd import retrieval as R
    e8, e32 = torch.zeros(0, 128, dtype=torch.int8, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)
    d2, dist, idx = R.knn_q8(e8, e32, dev(kq.random_rows(5, 1)), dev(kq.sq(kq.random_rows(5, 1))), k=3, scale=SCALE)
    assert d2.shape == dist.shape == idx.shape == (0, 3)


def test_determinism_and_streams():
    from affnet_amd import retrieval as R
    q, db = kq.random_rows(257, 31), kq.random_rows(1000, 32)
    want = kq.expected(kq.dist2(q, db), 8, SCALE, (100, 50))
    args = (dev(q), dev(kq.sq(q)), dev(db), dev(kq.sq(db)))
    runs = [R.knn_q8(*args, k=8, scale=SCALE, skip=(100, 50)) for _ in range(2)]
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
    with torch.cuda.stream(s):
        runs.append(R.knn_q8(*args, k=8, scale=SCALE, skip=(100, 50), n_chunks=3))
        x = dev(quantiser_input(65, SCALE))
        qq = R.quantize(x, SCALE)
    s.synchronize()
    for got in runs:
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        assert all(same(g.cpu().numpy(), w) for g, w in zip(got, want))
    assert same(qq[0].cpu().numpy(), kq.quantize(quantiser_input(65, SCALE), np.float32(SCALE))[0])


# ---- the quantised index against the fp32 one ----

def test_shortlist_equals_the_fp32_index_on_the_vote_fixture():
    from affnet_amd import retrieval as R
    v = kf.vote_setup()
    descs = [dev(d) for d in v["descs"]]
    fp32, q8 = R.DescriptorIndex(descs), R.QuantizedDescriptorIndex(descs)
    lean = R.QuantizedDescriptorIndex(descs, keep_float=False)
    scale = float(np.float32(127.0 / float(np.abs(v["D"]).max())))
    assert q8.scale == lean.scale == scale and q8.counts == kf.VOTE_COUNTS and lean.D is None and q8.D is not None
    want_q, want_sq = kq.quantize(v["D"], scale)
    assert same(q8.Dq.cpu().numpy(), want_q) and same(q8.sq.cpu().numpy(), want_sq) and same(lean.Dq.cpu().numpy(), want_q)
    bound = np.sqrt(128.0) / scale + 1e-3
    for s in (1, 3, 5, 7):
        q = dev(v["queries"][s])
        for k in (2, 4, 8):
            want = fp32.shortlist(q, k=k)
            assert want == ([s], [kf.VOTE_COUNTS[s]])
            assert q8.shortlist(q, k=k) == want and lean.shortlist(q, k=k) == want, (s, k)
            assert q8.shortlist(q, k=k, exclude=s) == fp32.shortlist(q, k=k, exclude=s) == ([], [])
            assert q8.shortlist(q, k=k, exclude=0) == fp32.shortlist(q, k=k, exclude=0)
        votes, dist, idx = q8.enqueue_votes(q, k=8)
        votes2, dist2, idx2 = lean.enqueue_votes(q, k=8)
        assert torch.equal(votes, votes2) and torch.equal(dist, dist2) and torch.equal(idx, idx2), "keep_float=False searches identically"
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        # the device's lists are the mirror's, and every reported distance is within the bound of the float64 distance of that pair
        want = kq.expected(kq.dist2(kq.quantize(v["queries"][s], scale)[0], want_q), 8, scale)
        assert same(dist, want[1]) and same(idx, want[2])
        D64 = kf.distance(v["queries"][s], v["D"])
        err = np.abs(dist.astype(np.float64) - np.take_along_axis(D64, idx.astype(np.int64), 1)).max()
        print("query %d: max |dist - float64 distance| = %.4f (bound %.4f)" % (s, err, bound))
        assert err <= bound
    with pytest.raises(ValueError, match="keep_float=False"):
        lean.retrieve(dev(v["queries"][1]), torch.zeros(45, 2, 3, device=DEV))
    with pytest.raises(ValueError, match="without LAFs"):
        q8.retrieve(dev(v["queries"][1]), torch.zeros(45, 2, 3, device=DEV))
    # a given scale is taken as it is
    assert R.QuantizedDescriptorIndex(descs, scale=100.0).scale == 100.0


COUNTS = [1, 15, 16, 17, 63, 64, 65, 130, 200]
_SET = {}


def image_set():
    """The ragged image set with frames that tests/test_gpu_knn.py retrieves from, made the same way (default_rng(11): unit descriptors that are
    noisy copies of rows of one pool of 200 unit vectors, random frames), computed once and never modified."""
    if not _SET:
        rng = np.random.default_rng(11)
        pool = rng.normal(size=(200, 128))
        descs, lafs = [], []
        for n in COUNTS:
            d = pool[rng.permutation(200)[:n]] + 0.06 * rng.normal(size=(n, 128))
            descs.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
            lafs.append(sp.random_frames(rng, n).astype(np.float32))
        _SET.update(descs=[dev(d) for d in descs], lafs=[dev(l) for l in lafs])
    return _SET


def test_retrieve_equals_the_fp32_index():
    from affnet_amd import retrieval as R
    from affnet_amd import ReprojectionStuff as RS
    s = image_set()
    descs, lafs = s["descs"], s["lafs"]
    fp32, q8 = R.DescriptorIndex(descs, lafs), R.QuantizedDescriptorIndex(descs, lafs)
    assert torch.equal(q8.D, fp32.D) and torch.equal(q8.L, fp32.L)
    for query, exclude in ((7, None), (7, 7), (4, 4)):
        assert q8.shortlist(descs[query], top=5, exclude=exclude) == fp32.shortlist(descs[query], top=5, exclude=exclude)
        want = fp32.retrieve(descs[query], lafs[query], top=5, exclude=exclude)
        res = q8.retrieve(descs[query], lafs[query], top=5, exclude=exclude)
        assert len(want) >= 2 and [r["image"] for r in res] == [r["image"] for r in want]
        for r, w in zip(res, want):
            assert sorted(r) == sorted(w) and (r["votes"], r["num_inliers"]) == (w["votes"], w["num_inliers"])
            for key in ("H", "tent_in_1", "tent_in_2", "inliers"):
                assert r[key].dtype == w[key].dtype and same(r[key].cpu().numpy(), w[key].cpu().numpy()), key
            t1, t2, H, inl, info = RS.match_and_verify(descs[query], descs[r["image"]], lafs[query], lafs[r["image"]])
            assert torch.equal(r["tent_in_1"], t1) and torch.equal(r["tent_in_2"], t2) and same(r["H"].cpu().numpy(), H.cpu().numpy())
            assert torch.equal(r["inliers"], inl) and r["num_inliers"] == info["num_inliers"]
