"""MI355X: the inverted-file search (csrc/ivf.hip affnet_ivf_search / affnet_ivf_cell_means / affnet_ivf_sqnorm, affnet_amd/retrieval.py).
With every cell probed the lists are affnet_knn's bytes; with fewer they are the restriction (tests/_ivf.py) of the device's own distance
matrix to the probed cells' rows, bytes again (so the squared norms of the cell-ordered copy carry affnet_knn's bits: one ulp in a norm would
move most distances); groups across every row-block edge; the edges; the codebook update against float64; the Python layer down to retrieve.
The data is tests/test_gpu_knn.py's: duplicate rows, self-copies and NaN self-distances."""
import numpy as np
import pytest
import torch

import _ivf as iv
import _knn_fp64 as kf
import test_gpu_knn as tk
import test_gpu_match_many as mm

pytestmark = pytest.mark.gpu

DEV = mm.DEV
SENT_F32, SENT_I32 = mm.SENT_F32, mm.SENT_I32
same, dev = mm.same, tk.dev


def make_parts(db, cells, centroids):
    """The tables of an index over db (numpy) for a GIVEN assignment and GIVEN centroids (neither has to be k-means' own), laid out on the host;
    the squared norms by affnet_ivf_sqnorm."""
    lib, ptr, check, ctx, st, d = mm._api()
    n2, nc = db.shape[0], centroids.shape[0]
    perm, start = iv.layout(np.asarray(cells, np.int64), nc)
    p = dict(n2=n2, n_cells=nc, cells=np.asarray(cells), perm=dev(perm), cell_start=dev(start), centroids=dev(centroids.astype(np.float32)),
             sorted=dev(db[perm].reshape(n2, 128)), sorted_sq=mm.full((max(n2, 1) + 2,), SENT_F32, torch.float32))
    if n2:
        check(lib.affnet_ivf_sqnorm(ctx, ptr(p["sorted"]), n2, 128, ptr(p["sorted_sq"]), st), ctx, "affnet_ivf_sqnorm")
        assert (p["sorted_sq"][n2:] == SENT_F32).all()
    return p


def raw_ivf(q, p, k, nprobe, skip=(0, 0), want_probes=True):
    """affnet_ivf_search on a device query -> numpy (dist (n1,k), idx (n1,k), probes (n1,nprobe)); the outputs are pre-filled with sentinels and
    two rows longer than n1."""
    lib, ptr, check, ctx, st, d = mm._api()
    n1, n2 = q.size(0), p["n2"]
    dist, idx = mm.full((n1 + 2, k), SENT_F32, torch.float32), mm.full((n1 + 2, k), SENT_I32, torch.int32)
    probes = mm.full((n1 + 2, nprobe), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_ivf_scratch_bytes(n1, p["n_cells"], nprobe, k), dtype=torch.uint8, device=d)
    one = torch.zeros(8, dtype=torch.float32, device=d)
    rc = lib.affnet_ivf_search(ctx, ptr(q if n1 else one), n1, ptr(p["sorted"] if n2 else one), ptr(p["sorted_sq"]), ptr(p["perm"] if n2 else one), n2,
                               ptr(p["cell_start"]), ptr(p["centroids"]), p["n_cells"], 128, k, nprobe, skip[0], skip[1], ptr(dist), ptr(idx),
                               ptr(probes) if want_probes else None, ptr(scratch), st)
    check(rc, ctx, "affnet_ivf_search")
    dist, idx, probes = dist.cpu().numpy(), idx.cpu().numpy(), probes.cpu().numpy()
    assert (dist[n1:] == SENT_F32).all() and (idx[n1:] == SENT_I32).all() and (probes[n1:] == SENT_I32).all(), "rows behind n1 stay untouched"
    if not want_probes:
        assert (probes == SENT_I32).all()
    return dist[:n1], idx[:n1], probes[:n1]


def random_cells(n2, n_cells, seed):
    """Rows assigned to cells at random, cell 1 left empty when there are at least 3 cells; arbitrary centroids."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, n_cells, n2)
    if n_cells >= 3:
        cells[cells == 1] = 2
    return cells, rng.normal(size=(n_cells, 128)).astype(np.float32) / 11.0


CASES = [(1, 1, 1), (15, 15, 2), (17, 17, 8), (63, 33, 1), (65, 415, 8), (130, 415, 3), (130, 1, 8), (1, 415, 8)]


@pytest.mark.parametrize("n1,n2,k", CASES)
def test_all_cells_probed_is_affnet_knn(n1, n2, k):
    _, db, q, ddb = tk.data(n1, n2)
    skips = ((0, 0), (n2 // 4, max(n2 // 2, 1)), (-3, 5), (n2 - 2, 10), (0, n2))          # random cells: every range crosses cell borders
    want = {skip: tk.raw_knn(q, ddb, k, skip) for skip in skips}
    for n_cells in (1, 3, 8):
        cells, cent = random_cells(n2, n_cells, 100 * n1 + n_cells)
        p = make_parts(db, cells, cent)
        if n_cells >= 3:
            start = p["cell_start"].cpu().numpy()
            assert start[1] == start[2], "cell 1 is empty"
        for skip in skips:
            want_d, want_i = want[skip]
            dist, idx, probes = raw_ivf(q, p, k, 8, skip)
            assert same(idx, want_i), (n_cells, skip, np.argwhere(idx != want_i)[:4])
            assert same(dist, want_d), (n_cells, skip)
            assert sorted(probes[0, :min(n_cells, 8)].tolist()) == list(range(min(n_cells, 8))) and (probes[:, n_cells:] == -1).all()


SIZES = [0, 1, 15, 16, 17, 33, 64, 100, 5, 48, 116]          # rows per cell: empty, one row, one below / at / one above the 16-column tile


_RESTRICTED = {}


def restricted_setup():
    """n1 = 130, n2 = 415 in 11 cells of SIZES, made once: the rows go to the cells at random; the centroid of a cell is its mean, except that the
    empty cell 0, the one-row cell 1 and the five-row cell 8 take the query rows 6, 3 and 4 as centroids - those rows probe them first."""
    if not _RESTRICTED:
        n1, n2 = 130, 415
        qn, db, q, ddb = tk.data(n1, n2)
        assert sum(SIZES) == n2
        rng = np.random.default_rng(77)
        cells = np.repeat(np.arange(len(SIZES)), SIZES)[rng.permutation(n2)]
        cent = np.zeros((len(SIZES), 128), np.float32)
        for c in range(len(SIZES)):
            if SIZES[c]:
                cent[c] = db[cells == c].astype(np.float64).mean(0)
        cent[0], cent[1], cent[8] = qn[6], qn[3], qn[4]
        _RESTRICTED.update(q=q, db=db, ddb=ddb, cells=cells, cent=cent, p=make_parts(db, cells, cent), M=tk.matrix(n1, n2))
    return _RESTRICTED


@pytest.mark.parametrize("nprobe", [1, 2, 5, 8])
def test_restricted_search(nprobe):
    s = restricted_setup()
    p, M = s["p"], s["M"]
    start = p["cell_start"].cpu().numpy()
    assert (np.diff(start) == SIZES).all()
    want_probes = tk.raw_knn(s["q"], p["centroids"], nprobe)[1]
    assert want_probes[6, 0] == 0 and want_probes[3, 0] == 1 and want_probes[4, 0] == 8, "the planted centroids are the rows' nearest"
    short = 0
    for k in (1, 3, 8):
        for skip in ((0, 0), (100, 200)):
            dist, idx, probes = raw_ivf(s["q"], p, k, nprobe, skip)
            assert same(probes, want_probes)
            want_d, want_i = iv.restricted_knn(M, s["cells"], probes, k, skip)
            assert same(idx, want_i), (k, skip, np.argwhere(idx != want_i)[:4])
            assert same(dist, want_d), (k, skip)
            short += int((want_i[:, k - 1] == -1).sum())
            if nprobe == 1 and skip == (0, 0):
                assert (idx[6] == -1).all() and np.isposinf(dist[6]).all(), "row 6 looks at the empty cell only"
                assert idx[3, 0] >= 0 and (idx[3, 1:] == -1).all(), "row 3 looks at the one-row cell only"
                assert (idx[4, :min(k, 5)] >= 0).all() and (idx[4, 5:] == -1).all(), "row 4 looks at the five-row cell only"
    if nprobe == 1:
        assert short >= 3, "the fixture has rows with fewer than k candidates"
    # the optional output left out: the same lists
    a, b = raw_ivf(s["q"], p, 3, nprobe), raw_ivf(s["q"], p, 3, nprobe, want_probes=False)
    assert same(a[0], b[0]) and same(a[1], b[1])


def test_fewer_cells_than_probes():
    s = restricted_setup()
    cells, cent = random_cells(415, 3, 9)
    p = make_parts(s["db"], cells, cent)
    for k in (1, 3, 8):
        dist, idx, probes = raw_ivf(s["q"], p, k, 8)
        assert same(probes[:, :3], tk.raw_knn(s["q"], p["centroids"], 3)[1]) and (probes[:, 3:] == -1).all()
        want_d, want_i = iv.restricted_knn(s["M"], cells, probes, k)
        assert same(idx, want_i) and same(dist, want_d), k
        assert same(idx, kf.sorted_knn(s["M"], k)[1])


@pytest.mark.parametrize("n1", [1, 15, 16, 17, 63, 64, 65, 130])
def test_group_sizes(n1):
    """Two cells, the second centroid far away: every query row probes cell 0, so the one group has n1 rows and crosses every edge of the
    16-row blocks; the rows of cell 1 are never looked at."""
    n2 = 415
    _, db, q, ddb = tk.data(n1, n2)
    rng = np.random.default_rng(n1)
    cells = (rng.random(n2) < 0.3).astype(np.int64)
    cent = np.stack([np.zeros(128, np.float32), np.full(128, 100.0, np.float32)])
    p = make_parts(db, cells, cent)
    M = tk.matrix(n1, n2)
    for k in (2, 8):
        dist, idx, probes = raw_ivf(q, p, k, 1, (7, 3))
        assert (probes == 0).all()
        want_d, want_i = iv.restricted_knn(M, cells, probes, k, (7, 3))
        assert same(idx, want_i) and same(dist, want_d), k
        assert (cells[idx[idx >= 0]] == 0).all()


def test_one_large_cell():
    """A degenerate codebook: every row in one cell of three, every query row in its group (9 row blocks x 26 tiles)."""
    s = restricted_setup()
    cells = np.full(415, 2)
    p = make_parts(s["db"], cells, np.stack([np.full(128, 100.0), np.full(128, -100.0), np.zeros(128)]))
    dist, idx, probes = raw_ivf(s["q"], p, 8, 2)
    assert (probes[:, 0] == 2).all()
    want_d, want_i = kf.sorted_knn(s["M"], 8)
    assert same(idx, want_i) and same(dist, want_d)


def test_edges_and_repeatability():
    lib, ptr, check, ctx, st, d = mm._api()
    s = restricted_setup()
    p = s["p"]
    # no query row: nothing is written
    dist, idx, probes = raw_ivf(s["q"][:0], p, 8, 8)
    assert dist.shape == (0, 8)
    # no database row: unfilled slots only
    empty = make_parts(np.zeros((0, 128), np.float32), np.zeros(0, np.int64), s["cent"])
    for nprobe in (1, 8):
        dist, idx, probes = raw_ivf(s["q"], empty, 3, nprobe)
        assert (idx == -1).all() and np.isposinf(dist).all() and (probes >= 0).all()
    # the same call twice: the grouping's atomics may order a group differently, the result cannot differ
    for k, nprobe in ((8, 5), (2, 8), (1, 1)):
        a, b = raw_ivf(s["q"], p, k, nprobe, (50, 60)), raw_ivf(s["q"], p, k, nprobe, (50, 60))
        assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2])
    # a refused call writes nothing
    buf = mm.full((64,), SENT_I32, torch.int32)
    for bad in (dict(k=0), dict(k=9), dict(np=0), dict(np=9), dict(dim=64), dict(nc=0)):
        a = dict(dict(k=8, np=8, dim=128, nc=11), **bad)
        rc = lib.affnet_ivf_search(ctx, ptr(s["q"]), 130, ptr(p["sorted"]), ptr(p["sorted_sq"]), ptr(p["perm"]), 415, ptr(p["cell_start"]),
                                   ptr(p["centroids"]), a["nc"], a["dim"], a["k"], a["np"], 0, 0, ptr(buf), ptr(buf), ptr(buf), ptr(buf), st)
        assert rc == -1 and b"ivf" in lib.affnet_last_error(ctx), bad
    torch.cuda.synchronize()
    assert (buf == SENT_I32).all()


def raw_cell_means(x, cells, cent):
    lib, ptr, check, ctx, st, d = mm._api()
    nc = cent.shape[0]
    perm, start = iv.layout(cells, nc)
    out = mm.full((nc + 1, 128), SENT_F32, torch.float32)
    out[:nc] = dev(cent)
    d_x, d_perm, d_start = dev(x), dev(perm), dev(start)          # named: a temporary's memory would be handed to the next one in front of the launch
    check(lib.affnet_ivf_cell_means(ctx, ptr(d_x), x.shape[0], 128, ptr(d_perm), ptr(d_start), nc, ptr(out), st), ctx, "affnet_ivf_cell_means")
    out = out.cpu().numpy()
    assert (out[nc] == SENT_F32).all()
    return out[:nc]


def test_cell_means():
    _, db, _, _ = tk.data(130, 415)          # rows of norm 1 and of norm 16 in the same cells
    cells, cent = random_cells(415, 11, 3)
    assert (cells == 1).sum() == 0 and np.bincount(cells, minlength=11).max() > 16
    got = raw_cell_means(db, cells, cent)
    want = iv.cell_means(db, cells, cent).astype(np.float32)
    # a double sum of at most 2^20 terms errs by far less than 2^-24 relatively, so the two roundings to fp32 differ by one ulp at most
    print("cell means: worst |got - want| = %.3g" % np.abs(got.astype(np.float64) - want).max())
    ok = (got == want) | (got == np.nextafter(want, np.float32(-np.inf))) | (got == np.nextafter(want, np.float32(np.inf)))
    assert ok.all(), np.argwhere(~ok)[:4]
    print("cell means: %d of %d entries differ from the float64 mean by one ulp" % ((got != want).sum(), got.size))
    assert same(got[1], cent[1]), "an empty cell keeps its centroid"
    assert same(got, raw_cell_means(db, cells, cent)), "two runs, equal bytes"


def test_train_cells():
    from affnet_amd import retrieval as R
    v = kf.vote_setup()
    D = dev(v["D"])
    a, b = R.train_cells(D, 8).cpu().numpy(), R.train_cells(D, 8).cpu().numpy()
    assert a.shape == (8, 128) and a.dtype == np.float32 and same(a, b), "two trainings, equal bytes"
    c0 = v["D"][iv.initial_rows(len(v["D"]), 8)]
    assert same(R.train_cells(D, 8, iters=0).cpu().numpy(), c0), "the init rule"
    f0, f1, f10 = iv.objective(v["D"], c0), iv.objective(v["D"], R.train_cells(D, 8, iters=1).cpu().numpy()), iv.objective(v["D"], a)
    print("k-means objective: initial %.4f, 1 iteration %.4f, 10 iterations %.4f" % (f0, f1, f10))
    assert f10 < f1 < f0
    # one step against the float64 restatement (the assignment of unit random rows has margins far above the fp32 error)
    want = iv.lloyd_step(v["D"], c0).astype(np.float32)
    got = R.train_cells(D, 8, iters=1).cpu().numpy()
    assert np.abs(got - want).max() <= np.spacing(np.abs(want).max())
    # a sample at a fixed stride: rows 0, 3, 6, ...
    s = R.train_cells(D, 4, iters=0, train_rows=200).cpu().numpy()
    sub = v["D"][::3]
    assert same(s, sub[iv.initial_rows(len(sub), 4)])


def _index_cells(index):
    perm, start = index.ivf.perm.cpu().numpy(), index.ivf.cell_start.cpu().numpy()
    cell_of_row = np.empty(perm.size, np.int64)
    cell_of_row[perm] = np.repeat(np.arange(start.size - 1), np.diff(start))
    return cell_of_row


@pytest.mark.parametrize("s", [1, 3, 5, 7])
def test_index_votes(s):
    from affnet_amd import retrieval as R
    v = kf.vote_setup()
    M = len(kf.VOTE_COUNTS)
    descs = [dev(d) for d in v["descs"]]
    index = R.IVFDescriptorIndex(descs, n_cells=8, nprobe=2)
    assert index.n_cells == 8 and index.nprobe == 2 and same(index.D.cpu().numpy(), v["D"])
    cell_of_row = _index_cells(index)
    assert same(index.ivf.sorted.cpu().numpy(), v["D"][index.ivf.perm.cpu().numpy()])
    q = dev(v["queries"][s])
    votes, dist, idx = index.enqueue_votes(q, k=4, ratio=0.8)
    d2, i2, probes = R.ivf_knn(q, index, k=4, nprobe=2, return_probes=True)
    dist, idx, probes = dist.cpu().numpy(), idx.cpu().numpy(), probes.cpu().numpy()
    assert same(d2.cpu().numpy(), dist) and same(i2.cpu().numpy(), idx)
    # (a) the lists are the restriction of the device's own matrix to the index's own cells and probes; the votes are the rule on them
    want_d, want_i = iv.restricted_knn(tk.raw_matrix(q, index.D), cell_of_row, probes, 4)
    assert same(idx, want_i) and same(dist, want_d)
    assert votes.dtype == torch.int32 and votes.cpu().tolist() == kf.votes(dist, idx, np.float32(0.8), v["row_image"], M, np.float32).tolist()
    # (b) precondition, in float64 with the device's cells: every planted copy lies in a probed cell
    n = kf.VOTE_COUNTS[s]
    nearest = np.argmin(kf.distance(v["queries"][s][:n], v["D"]), 1)
    assert (v["row_image"][nearest] == s).all()
    found = (cell_of_row[nearest][:, None] == probes[:n]).any(1)
    assert found.all(), "the fixture no longer separates: %d of %d planted copies lie outside the probed cells" % ((~found).sum(), n)
    exact = R.DescriptorIndex(descs).enqueue_votes(q, k=4, ratio=0.8)[0]
    assert votes.cpu().tolist() == exact.cpu().tolist()
    assert votes.cpu().tolist() == [n if i == s else 0 for i in range(M)]
    # nprobe is an attribute
    index.nprobe = 8
    d8, i8 = index.enqueue_votes(q, k=4)[1:]
    want = tk.raw_knn(q, index.D, 4)
    assert same(d8.cpu().numpy(), want[0]) and same(i8.cpu().numpy(), want[1])


def test_index_shortlist_and_retrieve():
    from affnet_amd import retrieval as R
    v = kf.vote_setup()
    e = torch.zeros(0, 128, device=DEV)
    ragged = [e, dev(v["descs"][3]), e, dev(v["descs"][5]), e]
    exact, index = R.DescriptorIndex(ragged), R.IVFDescriptorIndex(ragged, n_cells=8, nprobe=8)
    assert index.counts == [0, 17, 0, 64, 0]
    for s in (3, 5):
        for exclude in (None, 1, 2, 3):
            assert index.shortlist(dev(v["queries"][s]), exclude=exclude) == exact.shortlist(dev(v["queries"][s]), exclude=exclude)
    assert index.shortlist(dev(v["queries"][5])) == ([3], [64])
    s = mm.image_set()
    n = len(mm.COUNTS)
    descs = [s["D"][s["off"][i]:s["off"][i + 1]] for i in range(n)] + [e]
    lafs = [s["L"][s["off"][i]:s["off"][i + 1]] for i in range(n)] + [torch.zeros(0, 2, 3, device=DEV)]
    exact, index = R.DescriptorIndex(descs, lafs), R.IVFDescriptorIndex(descs, lafs, n_cells=8, nprobe=8)
    for query, exclude in ((7, None), (7, 7), (4, 4)):
        assert index.shortlist(descs[query], top=5, exclude=exclude) == exact.shortlist(descs[query], top=5, exclude=exclude)
        got, want = index.retrieve(descs[query], lafs[query], top=5, exclude=exclude), exact.retrieve(descs[query], lafs[query], top=5, exclude=exclude)
        assert len(got) == len(want) >= 2
        for a, b in zip(got, want):
            assert (a["image"], a["votes"], a["num_inliers"]) == (b["image"], b["votes"], b["num_inliers"])
            for key in ("H", "tent_in_1", "tent_in_2", "inliers"):
                assert torch.equal(a[key], b[key]) and a[key].dtype == b[key].dtype
    with pytest.raises(ValueError):
        R.IVFDescriptorIndex(descs).retrieve(descs[7], lafs[7])
