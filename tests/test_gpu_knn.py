"""MI355X: the descriptor index (csrc/knn.hip affnet_knn / affnet_knn_vote, affnet_amd/retrieval.py).  The k-nearest lists against the device's
own distance matrix sorted on the host (every reported distance is that matrix's element, so the comparison is on the bytes, NaNs included, and
for every number of column chunks), column 0 against the matcher, the skip range, unfilled slots, a float64 leg that does not go through the
device's matrix, the votes against the float64 restatement (tests/_knn_fp64.py) and against the rule recomputed from the device's own lists,
and the Python layer down to the batched verification."""
import os

import numpy as np
import pytest
import torch

import _knn_fp64 as kf
import test_gpu_match_many as mm

pytestmark = pytest.mark.gpu

DEV = mm.DEV
SENT_F32, SENT_I32 = mm.SENT_F32, mm.SENT_I32
same = mm.same
NCH = [0, 1, 2, 3, 7, 30]          # 30 > the 26 tiles of n2 = 415: some chunks are empty
FP64_BAR = 2e-6 * 2 + 1e-5         # tests/test_gpu_parity.py: the distance matrix against the oracle


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def raw_knn(q, db, k, skip=(0, 0), nc=0):
    """affnet_knn on two device tensors -> numpy (dist (n1,k), idx (n1,k)), the outputs pre-filled with sentinels."""
    lib, ptr, check, ctx, st, d = mm._api()
    n1, n2 = q.size(0), db.size(0)
    dist, idx = mm.full((max(n1, 1), k), SENT_F32, torch.float32), mm.full((max(n1, 1), k), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_knn_scratch_bytes(n1, n2, k, nc), dtype=torch.uint8, device=d)
    one = torch.zeros(8, dtype=torch.float32, device=d)
    check(lib.affnet_knn(ctx, ptr(q if n1 else one), n1, ptr(db if n2 else one), n2, 128, k, skip[0], skip[1], nc, ptr(dist), ptr(idx), ptr(scratch), st), ctx, "affnet_knn")
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert (dist[n1:] == SENT_F32).all() and (idx[n1:] == SENT_I32).all()
    return dist[:n1], idx[:n1]


def raw_matrix(q, db):
    lib, ptr, check, ctx, st, d = mm._api()
    n1, n2 = q.size(0), db.size(0)
    out = mm.full((n1, n2), SENT_F32, torch.float32)
    scratch = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=d)
    check(lib.affnet_distance_matrix(ctx, ptr(q), n1, ptr(db), n2, 128, ptr(out), ptr(scratch), st), ctx, "affnet_distance_matrix")
    return out.cpu().numpy()


def raw_votes(dist, idx, ratio, row_image, n_images):
    lib, ptr, check, ctx, st, d = mm._api()
    n1, k = idx.shape
    votes = mm.full((n_images + 3,), SENT_I32, torch.int32)
    d_dist, d_idx, d_ri = dev(np.asarray(dist, np.float32)), dev(np.asarray(idx, np.int32)), dev(np.asarray(row_image, np.int32))
    if n1 == 0:          # an empty tensor has no storage, and the boundary refuses NULL
        d_dist, d_idx = torch.zeros(8, dtype=torch.float32, device=d), torch.zeros(8, dtype=torch.int32, device=d)
    check(lib.affnet_knn_vote(ctx, ptr(d_dist), ptr(d_idx), n1, k, ratio, ptr(d_ri), len(row_image), n_images, ptr(votes), st), ctx, "affnet_knn_vote")
    votes = votes.cpu().numpy()
    assert (votes[n_images:] == SENT_I32).all()
    return votes[:n_images]


_DATA = {}


def data(n1, n2, planted=True):
    """Query and database of one size, made once and never modified: noisy copies of rows of one pool of 200 unit vectors, as
    test_gpu_match_many.image_set makes them.  planted: the database also holds exact duplicate rows (equal distances: the row index decides)
    and some query rows are database rows themselves (near-zero distances), one of them a duplicated row; half of those rows are 16 times as
    long as the rest, which is where the self-distances come out NaN (test_against_the_sorted_distance_matrix prints how many)."""
    key = (n1, n2, planted)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * n1 + n2)
        pool = rng.normal(size=(200, 128))

        def noisy(n):
            d = pool[rng.integers(0, 200, n)] + 0.06 * rng.normal(size=(n, 128))
            return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        q, db = noisy(n1), noisy(n2)
        if planted and n2 >= 4:
            # long rows: at |b|^2 = 256 the fp32 expansion of a self-distance is off by many times 1e-6, below -1e-6 (NaN) as often as not
            db[0] *= 16.0
            for i in range(0, n1, 10):
                db[(7 * i) % n2] *= 16.0
            db[n2 - 1] = db[0]
            db[n2 // 2] = db[1]
            if n2 >= 40:
                db[37] = db[20]
                db[n2 - 2] = db[20]
            for i in range(0, n1, 5):
                q[i] = db[(7 * i) % n2]
            q[n1 - 1] = db[0]
        _DATA[key] = (q, db, dev(q), dev(db))
    return _DATA[key]


_MATRIX = {}


def matrix(n1, n2):
    if (n1, n2) not in _MATRIX:
        _, _, q, db = data(n1, n2)
        _MATRIX[(n1, n2)] = raw_matrix(q, db)
    return _MATRIX[(n1, n2)]


# every n1, n2 and k of the issue appears, and each case runs with every n_chunks
CASES = [(1, 1, 1), (15, 15, 2), (16, 16, 3), (17, 17, 8), (63, 33, 1), (64, 200, 2), (65, 415, 8), (130, 415, 3), (130, 1, 8), (1, 415, 8),
         (64, 16, 8), (17, 200, 1), (65, 33, 3), (16, 415, 2), (15, 200, 8), (63, 415, 1)]


@pytest.mark.parametrize("n1,n2,k", CASES)
def test_against_the_sorted_distance_matrix(n1, n2, k):
    _, _, q, db = data(n1, n2)
    M = matrix(n1, n2)
    want_d, want_i = kf.sorted_knn(M, k)
    print("%d x %d: %d NaN distances, %d rows with more than one" % (n1, n2, np.isnan(M).sum(), (np.isnan(M).sum(1) > 1).sum()))
    for nc in NCH:
        dist, idx = raw_knn(q, db, k, nc=nc)
        assert same(idx, want_i), (nc, np.argwhere(idx != want_i)[:4])
        assert same(dist, want_d), nc
    if n2 >= 40 and n1 >= 15:
        assert (M[n1 - 1, 0] == M[n1 - 1, n2 - 1]) or np.isnan(M[n1 - 1, 0]), "a duplicated database row gives equal distances"


@pytest.mark.parametrize("i,j", [(0, 8), (3, 5), (7, 8), (8, 7), (6, 2), (4, 4)])
def test_k1_is_the_matcher(i, j):
    s = mm.image_set()
    a, b = s["D"][s["off"][i]:s["off"][i + 1]], s["D"][s["off"][j]:s["off"][j + 1]]
    want = mm.raw_snn(a, b)
    for nc in NCH:
        dist, idx = raw_knn(a, b, 1, nc=nc)
        assert same(dist[:, 0], want["md"]) and same(idx[:, 0], want["idx"]), (i, j, nc)
    _, _, q, db = data(130, 415)          # with planted self-copies and duplicates
    want = mm.raw_snn(q, db)
    dist, idx = raw_knn(q, db, 1)
    assert same(dist[:, 0], want["md"]) and same(idx[:, 0], want["idx"])


# n2 = 415, n_chunks = 3: 26 tiles, 9 per chunk, so chunk 1 owns columns [144, 288)
SKIPS = [(18, 5),          # inside one tile
         (140, 10),        # straddles two tiles and the boundary of chunks 0 / 1
         (144, 144),       # a whole chunk
         (0, 415),         # everything
         (100, 0),         # no skip
         (400, 100),       # reaches past n2
         (-5, 10),         # starts in front of 0
         (500, 3)]         # behind n2 altogether


@pytest.mark.parametrize("skip", SKIPS)
def test_skip_range(skip):
    n1, n2 = 65, 415
    _, _, q, db = data(n1, n2)
    M = matrix(n1, n2)
    for k in (3, 8):
        want_d, want_i = kf.sorted_knn(M, k, skip)
        lo, hi = max(skip[0], 0), skip[0] + skip[1]
        assert not ((want_i >= lo) & (want_i < hi)).any()
        if skip == (0, 415):
            assert (want_i == -1).all() and np.isposinf(want_d).all()
        for nc in NCH:
            dist, idx = raw_knn(q, db, k, skip, nc)
            assert same(idx, want_i) and same(dist, want_d), (skip, k, nc)


def test_fewer_candidates_than_k():
    q, db, dq, ddb = data(17, 415)
    M = matrix(17, 415)
    for nc in NCH:
        dist, idx = raw_knn(dq, ddb[:3].contiguous(), 8, nc=nc)
        want_d, want_i = kf.sorted_knn(M[:, :3], 8)          # column c of the matrix depends on database row c alone
        assert same(idx, want_i) and same(dist, want_d), nc
        assert (idx[:, 3:] == -1).all() and np.isposinf(dist[:, 3:]).all() and (idx[:, :3] >= 0).all()
        dist, idx = raw_knn(dq, ddb[:0], 8, nc=nc)
        assert idx.shape == (17, 8) and (idx == -1).all() and np.isposinf(dist).all(), nc
        # two candidates left by the skip range
        dist, idx = raw_knn(dq, ddb[:3].contiguous(), 2, (1, 1), nc)
        assert same(idx, kf.sorted_knn(M[:, :3], 2, (1, 1))[1]) and set(idx.ravel().tolist()) == {0, 2}
    # no query row: nothing is written
    lib, ptr, check, ctx, st, d = mm._api()
    buf = mm.full((64,), SENT_I32, torch.int32)
    assert lib.affnet_knn(ctx, ptr(dq), 0, ptr(ddb), 415, 128, 8, 0, 0, 0, ptr(buf), ptr(buf), ptr(buf), st) == 0
    for bad in (dict(k=0), dict(k=9), dict(dim=64), dict(nc=-1)):
        a = dict(dict(k=8, dim=128, nc=0), **bad)
        assert lib.affnet_knn(ctx, ptr(dq), 17, ptr(ddb), 415, a["dim"], a["k"], 0, 0, a["nc"], ptr(buf), ptr(buf), ptr(buf), st) == -1, bad
        assert b"knn" in lib.affnet_last_error(ctx)
    torch.cuda.synchronize()
    assert (buf == SENT_I32).all(), "a refused call writes nothing"


def _fp64_leg(q, db, k, ncs):
    want_d, _ = kf.sorted_knn(kf.distance(q, db), k)
    assert np.isfinite(want_d).all()
    worst = 0.0
    for nc in ncs:
        dist, _ = raw_knn(dev(q), dev(db), k, nc=nc)
        worst = max(worst, float(np.abs(dist.astype(np.float64) - want_d).max()))
    print("sorted distances against float64: worst |diff| %.3g (bar %.3g)" % (worst, FP64_BAR))
    assert worst < FP64_BAR


@pytest.mark.parametrize("n1,n2,k", [(130, 415, 8), (65, 200, 3), (17, 33, 2), (64, 415, 1)])
def test_float64_leg(n1, n2, k):
    """Independent of the device's own matrix: the sorted distances (values, not indices, so a near-tie cannot flip the comparison) against the
    float64 restatement.  No planted self-copies here: at a distance of ~1e-3 the fp32 expansion is not good to the bar."""
    q, db, _, _ = data(n1, n2, planted=False)
    _fp64_leg(q, db, k, NCH)


def test_float64_leg_on_graf_descriptors():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_graf16_n500.npz"))
    d1, d2 = np.ascontiguousarray(g["desc1"], np.float32), np.ascontiguousarray(g["desc2"], np.float32)
    _fp64_leg(d1, d2, 8, [0, 1, 5])
    dist, idx = raw_knn(dev(d1), dev(d2), 2)
    assert np.abs(dist[:, 0] - g["min_dist"]).max() < 1e-5
    assert (idx[:, 0] == g["idx"]).mean() > 0.99


def _vote_case(q, D, row_image, n_images, k, skip=(0, 0)):
    """The device's votes for query q against database D; they must equal the float64 restatement's (whose every comparison has a margin far above
    the fp32 error) and the rule recomputed in fp32 from the device's own lists.  Returns them."""
    want_d, want_i = kf.sorted_knn(kf.distance(q, D), k, skip)
    margin = kf.vote_margin(want_d, want_i, 0.8)
    assert margin > 1e-3, "a wrong input, not a case to leave out: margin %g" % margin
    want = kf.votes(want_d, want_i, 0.8, row_image, n_images)
    dist, idx = raw_knn(dev(q), dev(D), k, skip)
    got = raw_votes(dist, idx, 0.8, row_image, n_images)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert got.tolist() == kf.votes(dist, idx, np.float32(0.8), row_image, n_images, np.float32).tolist()
    return got


@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("s", [1, 3, 5, 7])
def test_votes(s, k):
    v = kf.vote_setup()
    M = len(kf.VOTE_COUNTS)
    got = _vote_case(v["queries"][s], v["D"], v["row_image"], M, k)
    want = np.zeros(M, np.int32)
    want[s] = kf.VOTE_COUNTS[s]
    assert got.tolist() == want.tolist()
    got = _vote_case(v["queries"][s], v["D"], v["row_image"], M, k, (int(v["off"][s]), kf.VOTE_COUNTS[s]))
    assert not got.any(), "without its source image the query votes for nobody"


def test_votes_special_cases():
    v = kf.vote_setup()
    M = len(kf.VOTE_COUNTS)
    # two database images that are noisy copies of the same source, k = 3: both receive the votes
    D = np.concatenate([v["D"], v["twin"]])
    row_image = np.concatenate([v["row_image"], np.full(len(v["twin"]), M, np.int32)])
    got = _vote_case(v["queries"][3], D, row_image, M + 1, 3)
    assert got[3] == got[M] == kf.VOTE_COUNTS[3] and got.sum() == 2 * kf.VOTE_COUNTS[3]
    # k = 1: all zeros (and the buffer IS zeroed)
    dist, idx = raw_knn(dev(v["queries"][3]), dev(v["D"]), 1)
    assert raw_votes(dist, idx, 0.8, v["row_image"], M).tolist() == [0] * M
    # ids out of range, planted: a database row beyond n2, a negative one other than -1, an image id beyond n_images and a negative one
    dist, idx = raw_knn(dev(v["queries"][3]), dev(v["D"]), 3)
    clean = raw_votes(dist, idx, 0.8, v["row_image"], M)
    assert clean[3] == kf.VOTE_COUNTS[3]
    idx2 = idx.copy()
    idx2[0, 0], idx2[1, 0], idx2[2, 0] = 10 ** 6, -5, len(v["row_image"])
    ri = v["row_image"].copy()
    ri[idx[3, 0]], ri[idx[4, 0]] = M, -3
    got = raw_votes(dist, idx2, 0.8, ri, M)
    assert got.tolist() == kf.votes(dist, idx2, np.float32(0.8), ri, M, np.float32).tolist()
    assert got[3] == clean[3] - 5 and got.sum() == clean.sum() - 5
    # no query row: the votes are still zeroed
    assert raw_votes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0.8, v["row_image"], M).tolist() == [0] * M


def test_python_layer_shortlist():
    from affnet_amd import retrieval as R
    v = kf.vote_setup()
    index = R.DescriptorIndex([dev(d) for d in v["descs"]])
    assert index.counts == kf.VOTE_COUNTS and index.offsets == v["off"].tolist() and index.L is None
    assert same(index.row_image.cpu().numpy(), v["row_image"]) and same(index.D.cpu().numpy(), v["D"])
    for s in (1, 3, 5, 7):
        q = dev(v["queries"][s])
        assert index.shortlist(q) == ([s], [kf.VOTE_COUNTS[s]])
        assert index.shortlist(q, exclude=s) == ([], [])
        assert index.shortlist(q, top=0) == ([], [])
    # the wrapper is the raw call; skip and n_chunks pass through
    q = dev(v["queries"][7])
    dist, idx = R.knn(q, index.D, k=3, skip=index.skip_range(7), n_chunks=3)
    want = raw_knn(q, index.D, 3, index.skip_range(7), 1)
    assert same(dist.cpu().numpy(), want[0]) and same(idx.cpu().numpy(), want[1]) and idx.dtype == torch.int32
    votes, dist, idx = index.enqueue_votes(q, k=3)
    assert votes.dtype == torch.int32 and votes.tolist() == [0] * 7 + [130, 0] and dist.shape == (160, 3)
    # an index with empty images
    e = torch.zeros(0, 128, device=DEV)
    ragged = R.DescriptorIndex([e, dev(v["descs"][3]), e, dev(v["descs"][5]), e])
    assert ragged.counts == [0, 17, 0, 64, 0] and ragged.shortlist(dev(v["queries"][5])) == ([3], [64])
    assert ragged.shortlist(dev(v["queries"][5]), exclude=2) == ([3], [64])
    with pytest.raises(ValueError):
        index.shortlist(q, exclude=9)
    with pytest.raises(ValueError):
        index.shortlist(q, k=9)
    with pytest.raises(ValueError):
        index.retrieve(q, torch.zeros(160, 2, 3, device=DEV))


def test_python_layer_retrieve():
    from affnet_amd import retrieval as R
    s = mm.image_set()
    RS = s["RS"]
    descs = [s["D"][s["off"][i]:s["off"][i + 1]] for i in range(len(mm.COUNTS))]
    lafs = [s["L"][s["off"][i]:s["off"][i + 1]] for i in range(len(mm.COUNTS))]
    index = R.DescriptorIndex(descs, lafs)
    assert same(index.L.cpu().numpy(), s["L"].cpu().numpy())
    for query, exclude in ((7, None), (7, 7), (4, 4)):
        images, votes = index.shortlist(descs[query], top=5, exclude=exclude)
        assert 2 <= len(images) <= 5 and votes == sorted(votes, reverse=True) and (query in images) == (exclude is None)
        res = index.retrieve(descs[query], lafs[query], top=5, exclude=exclude)
        assert sorted(r["image"] for r in res) == sorted(images) and [r["votes"] for r in res] == [votes[images.index(r["image"])] for r in res]
        n = [r["num_inliers"] for r in res]
        assert n == sorted(n, reverse=True), "by descending inliers"
        for a, b in zip(res, res[1:]):
            assert a["num_inliers"] > b["num_inliers"] or images.index(a["image"]) < images.index(b["image"]), "ties in shortlist order"
        for r in res:
            t1, t2, H, inl, info = RS.match_and_verify(descs[query], descs[r["image"]], lafs[query], lafs[r["image"]])
            assert torch.equal(r["tent_in_1"], t1) and torch.equal(r["tent_in_2"], t2) and r["tent_in_1"].dtype == torch.int64
            assert same(r["H"].cpu().numpy(), H.cpu().numpy()) and r["H"].dtype == torch.float64
            assert torch.equal(r["inliers"], inl) and r["inliers"].dtype == torch.bool and r["num_inliers"] == info["num_inliers"]
        if exclude is None:
            assert res[0]["image"] == query, "the query's own image has the query's own frames; every other image has random ones"
