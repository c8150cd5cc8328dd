"""MI355X: the inverted-file search over int8 rows (csrc/ivf.hip affnet_ivf_search_q8, affnet_amd/retrieval.py).  The arithmetic is integer
and exact and the order (d2, original row) is total, so every comparison is on the bytes of the outputs: with every cell probed they are
affnet_knn_q8's on the unpermuted rows; with fewer they are the restriction (tests/_ivf_q8.py) of the exact integer matrix to the probed cells'
rows, the cells being affnet_knn's on the float centroids and affnet_ivf_search's; groups across every row-block edge, cells across every edge
of the kernel's 64-column step and of the four waves' 256; the edges; the Python layer down to retrieve.
The database is tests/_knn_q8.py's random rows (asymmetric data); the tie fixture has rows over {-1, 0, 1} with exact duplicates in other cells."""
import numpy as np
import pytest
import torch

import _ivf as iv
import _ivf_q8 as iq
import _knn_fp64 as kf
import _knn_q8 as kq
import test_gpu_ivf as ti
import test_gpu_knn as tk
import test_gpu_knn_q8 as tq

pytestmark = pytest.mark.gpu

DEV = tq.DEV
SENT_F32, SENT_I32 = tq.SENT_F32, tq.SENT_I32
SCALE = tq.SCALE
same, dev, full = tq.same, tq.dev, tq.full


def as_float(q8):
    """The float rows an int8 array stands for at SCALE: what the coarse step reads (the raw call takes the two forms side by side)."""
    return (q8.astype(np.float32) / np.float32(SCALE)).astype(np.float32)


def make_parts(db8, cells, centroids):
    """The tables of an index over the int8 rows db8 (numpy) for a GIVEN assignment and GIVEN float centroids, laid out on the host."""
    n2, nc = db8.shape[0], centroids.shape[0]
    perm, start = iv.layout(np.asarray(cells, np.int64), nc)
    return dict(n2=n2, n_cells=nc, cells=np.asarray(cells), perm=dev(perm), cell_start=dev(start), centroids=dev(centroids.astype(np.float32)),
                sorted_q=dev(db8[perm].reshape(n2, 128)), sorted_sq=dev(kq.sq(db8)[perm].reshape(n2)))


def raw_ivf_q8(qf, q8, p, k, nprobe, skip=(0, 0), want_probes=True, scale=SCALE):
    """affnet_ivf_search_q8 on numpy queries (float rows for the coarse step, int8 rows for the cells) -> numpy (dist2, dist, idx (n1,k), probes
    (n1,nprobe)); the outputs are pre-filled with sentinels and two rows longer than n1."""
    lib, ptr, check, ctx, st, d = tq._api()
    n1, n2 = q8.shape[0], p["n2"]
    one = torch.zeros(16, dtype=torch.int32, device=d)          # stands in for empty inputs: never read, but the boundary refuses NULL
    dqf, dq8, dqs = (dev(qf), dev(q8), dev(kq.sq(q8))) if n1 else (one, one, one)
    d2, dist, idx = full((n1 + 2, k), SENT_I32, torch.int32), full((n1 + 2, k), SENT_F32, torch.float32), full((n1 + 2, k), SENT_I32, torch.int32)
    probes = full((n1 + 2, nprobe), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_ivf_q8_scratch_bytes(n1, p["n_cells"], nprobe, k), dtype=torch.uint8, device=d)
    rc = lib.affnet_ivf_search_q8(ctx, ptr(dqf), ptr(dq8), ptr(dqs), n1, ptr(p["sorted_q"] if n2 else one), ptr(p["sorted_sq"] if n2 else one),
                                  ptr(p["perm"] if n2 else one), n2, ptr(p["cell_start"]), ptr(p["centroids"]), p["n_cells"], 128, k, nprobe, skip[0], skip[1],
                                  scale, ptr(d2), ptr(dist), ptr(idx), ptr(probes) if want_probes else None, ptr(scratch), st)
    check(rc, ctx, "affnet_ivf_search_q8")
    d2, dist, idx, probes = d2.cpu().numpy(), dist.cpu().numpy(), idx.cpu().numpy(), probes.cpu().numpy()
    assert (d2[n1:] == SENT_I32).all() and (dist[n1:] == SENT_F32).all() and (idx[n1:] == SENT_I32).all() and (probes[n1:] == SENT_I32).all(), \
        "rows behind n1 stay untouched"
    if not want_probes:
        assert (probes == SENT_I32).all()
    return d2[:n1], dist[:n1], idx[:n1], probes[:n1]


def same3(got, want):
    return same(got[2], want[2]) and same(got[0], want[0]) and same(got[1], want[1])


# ---- 1. every cell probed: affnet_knn_q8's bytes ----

CASES = [(1, 1, 1), (15, 15, 2), (17, 17, 8), (63, 33, 1), (65, 415, 8), (130, 415, 3), (130, 1, 8), (1, 415, 8)]


@pytest.mark.parametrize("n1,n2,k", CASES)
def test_all_cells_probed_is_affnet_knn_q8(n1, n2, k):
    q8, db8 = kq.random_rows(n1, 1000 + n1), kq.random_rows(n2, 2000 + n2)
    M = kq.dist2(q8, db8)
    skips = ((0, 0), (n2 // 4, max(n2 // 2, 1)), (-3, 5), (n2 - 2, 10), (0, n2))          # random cells: every range crosses cell borders
    want = {skip: tq.raw_knn(q8, db8, k, skip) for skip in skips}
    for skip in skips:
        assert same3(want[skip], kq.expected(M, k, SCALE, skip)), skip
    for n_cells in (1, 3, 8):
        cells, cent = ti.random_cells(n2, n_cells, 100 * n1 + n_cells)
        p = make_parts(db8, cells, cent)
        if n_cells >= 3:
            start = p["cell_start"].cpu().numpy()
            assert start[1] == start[2], "cell 1 is empty"
        for skip in skips:
            got = raw_ivf_q8(as_float(q8), q8, p, k, 8, skip)
            assert same(got[2], want[skip][2]), (n_cells, skip, np.argwhere(got[2] != want[skip][2])[:4])
            assert same3(got, want[skip]), (n_cells, skip)
            assert sorted(got[3][0, :min(n_cells, 8)].tolist()) == list(range(min(n_cells, 8))) and (got[3][:, n_cells:] == -1).all()


_TIES = {}


def tie_setup():
    """n2 = 415 rows over {-1, 0, 1} in 8 random cells (cell 1 empty); every tenth row is an exact duplicate of another row that is ASSIGNED TO A
    DIFFERENT CELL, so the two stand at the same d2 from every query and only the order by original row across cells puts them right.  The 65
    queries: 33 database rows (d2 = 0 against both copies) and 32 more rows over {-1, 0, 1}.  Made once."""
    if not _TIES:
        rng = np.random.default_rng(41)
        n2 = 415
        db8 = rng.integers(-1, 2, size=(n2, 128)).astype(np.int8)
        cells, cent = ti.random_cells(n2, 8, 41)
        twins, free = [], np.arange(n2) % 10 != 9          # a row is copied once at most: every duplicate is a pair
        for r in range(9, n2, 10):
            s = int(rng.choice(np.nonzero((cells != cells[r]) & free)[0]))
            db8[r], free[s] = db8[s], False
            twins.append((r, s))
        q8 = np.concatenate([db8[[s for _, s in twins[:33]]], rng.integers(-1, 2, size=(32, 128)).astype(np.int8)])
        _TIES.update(db8=db8, q8=q8, cells=cells, cent=cent, twins=twins)
    return _TIES


@pytest.mark.parametrize("k", [2, 8])
def test_ties_across_cells_go_to_the_lower_original_row(k):
    t = tie_setup()
    db8, q8, cells = t["db8"], t["q8"], t["cells"]
    assert all(cells[r] != cells[s] and (db8[r] == db8[s]).all() for r, s in t["twins"])
    p = make_parts(db8, cells, t["cent"])
    M = kq.dist2(q8, db8)
    for skip in ((0, 0), (100, 200)):
        want = tq.raw_knn(q8, db8, k, skip)
        assert same3(want, kq.expected(M, k, SCALE, skip))
        got = raw_ivf_q8(as_float(q8), q8, p, k, 8, skip)
        assert same3(got, want), (skip, np.argwhere(got[2] != want[2])[:4])
    d2, dist, idx, _ = raw_ivf_q8(as_float(q8), q8, p, k, 8)
    for j, (r, s) in enumerate(t["twins"][:33]):          # the query is a copy of both: d2 = 0 twice, the lower original row first, from two cells
        assert d2[j, 0] == 0 and d2[j, 1] == 0 and idx[j, :2].tolist() == sorted((r, s)), j
    if k == 8:
        assert (d2[:, :-1] == d2[:, 1:]).sum() > 65, "the fixture is full of ties"
    assert ((d2[:, :-1] < d2[:, 1:]) | ((d2[:, :-1] == d2[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))).all()


# ---- 2. restricted search ----

# rows per cell: empty, one row, one below / at / one above 16, 32, 64 (the kernel's step), 128 and 256 (the four waves' steps); the five-row cell
SIZES = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 5, 255, 256, 257]
N2 = sum(SIZES)          # 1494

_RESTRICTED = {}


def restricted_setup():
    """n1 = 130, n2 = 1494 in 18 cells of SIZES, made once: the rows go to the cells at random; the centroid of a cell is the mean of its float
    rows, except that the empty cell 0, the one-row cell 1 and the five-row cell 14 take the query rows 6, 3 and 4 as centroids - those rows
    probe them first."""
    if not _RESTRICTED:
        n1 = 130
        q8, db8 = kq.random_rows(n1, 71), kq.random_rows(N2, 72)
        qf, dbf = as_float(q8), as_float(db8)
        rng = np.random.default_rng(77)
        cells = np.repeat(np.arange(len(SIZES)), SIZES)[rng.permutation(N2)]
        cent = np.zeros((len(SIZES), 128), np.float32)
        for c in range(len(SIZES)):
            if SIZES[c]:
                cent[c] = dbf[cells == c].astype(np.float64).mean(0)
        cent[0], cent[1], cent[14] = qf[6], qf[3], qf[4]
        _RESTRICTED.update(q8=q8, db8=db8, qf=qf, dbf=dbf, cells=cells, cent=cent, p=make_parts(db8, cells, cent), pf=ti.make_parts(dbf, cells, cent),
                           M=kq.dist2(q8, db8))
    return _RESTRICTED


def expected_from(M, cells, probes, k, skip=(0, 0)):
    d2, idx = iq.restricted_knn_int(M, cells, probes, k, skip)
    dist = np.where(idx >= 0, kq.fdist(np.where(idx >= 0, d2, 0), SCALE), np.float32(np.inf)).astype(np.float32)
    return d2, dist, idx


@pytest.mark.parametrize("nprobe", [1, 2, 5, 8])
def test_restricted_search(nprobe):
    s = restricted_setup()
    p, M = s["p"], s["M"]
    start = p["cell_start"].cpu().numpy()
    assert (np.diff(start) == SIZES).all() and SIZES[0] == 0 and SIZES[1] == 1 and SIZES[14] == 5
    want_probes = tk.raw_knn(dev(s["qf"]), p["centroids"], nprobe)[1]
    assert want_probes[6, 0] == 0 and want_probes[3, 0] == 1 and want_probes[4, 0] == 14, "the planted centroids are the rows' nearest"
    assert same(ti.raw_ivf(dev(s["qf"]), s["pf"], 3, nprobe)[2], want_probes), "affnet_ivf_search looks at the same cells"
    short = 0
    for k in (1, 3, 8):
        for skip in ((0, 0), (100, 200)):
            got = raw_ivf_q8(s["qf"], s["q8"], p, k, nprobe, skip)
            assert same(got[3], want_probes)
            want = expected_from(M, s["cells"], got[3], k, skip)
            assert same(got[2], want[2]), (k, skip, np.argwhere(got[2] != want[2])[:4])
            assert same3(got, want), (k, skip)
            short += int((want[2][:, k - 1] == -1).sum())
            if nprobe == 1 and skip == (0, 0):
                d2, dist, idx = got[:3]
                assert (idx[6] == -1).all() and np.isposinf(dist[6]).all() and (d2[6] == kq.INT32_MAX).all(), "row 6 looks at the empty cell only"
                assert idx[3, 0] >= 0 and (idx[3, 1:] == -1).all(), "row 3 looks at the one-row cell only"
                assert (idx[4, :min(k, 5)] >= 0).all() and (idx[4, 5:] == -1).all(), "row 4 looks at the five-row cell only"
    if nprobe == 1:
        assert short >= 3, "the fixture has rows with fewer than k candidates"
    # the optional output left out: the same lists
    a, b = raw_ivf_q8(s["qf"], s["q8"], p, 3, nprobe), raw_ivf_q8(s["qf"], s["q8"], p, 3, nprobe, want_probes=False)
    assert same3(a, b)


# ---- 3. group sizes ----

@pytest.mark.parametrize("n1", [1, 15, 16, 17, 63, 64, 65, 130])
def test_group_sizes(n1):
    """Two cells, the second centroid far away: every query row probes cell 0, so the one group has n1 rows and crosses every edge of the
    16-row blocks; the rows of cell 1 are never looked at."""
    n2 = 415
    q8, db8 = kq.random_rows(n1, 3000 + n1), kq.random_rows(n2, 2000 + n2)
    rng = np.random.default_rng(n1)
    cells = (rng.random(n2) < 0.3).astype(np.int64)
    cent = np.stack([np.zeros(128, np.float32), np.full(128, 100.0, np.float32)])
    p = make_parts(db8, cells, cent)
    M = kq.dist2(q8, db8)
    for k in (2, 8):
        got = raw_ivf_q8(as_float(q8), q8, p, k, 1, (7, 3))
        assert (got[3] == 0).all()
        want = expected_from(M, cells, got[3], k, (7, 3))
        assert same3(got, want), k
        assert (cells[got[2][got[2] >= 0]] == 0).all()


# ---- 4. degenerate codebooks ----

def test_one_large_cell():
    """Every row in one cell of three, every query row in its group (9 row blocks, 24 steps of 64 columns over the four waves)."""
    s = restricted_setup()
    cells = np.full(N2, 2)
    p = make_parts(s["db8"], cells, np.stack([np.full(128, 100.0), np.full(128, -100.0), np.zeros(128)]))
    got = raw_ivf_q8(s["qf"], s["q8"], p, 8, 2)
    assert (got[3][:, 0] == 2).all()
    assert same3(got, kq.expected(s["M"], 8, SCALE))


def test_fewer_cells_than_probes():
    s = restricted_setup()
    cells, cent = ti.random_cells(N2, 3, 9)
    p = make_parts(s["db8"], cells, cent)
    for k in (1, 3, 8):
        got = raw_ivf_q8(s["qf"], s["q8"], p, k, 8)
        assert same(got[3][:, :3], tk.raw_knn(dev(s["qf"]), p["centroids"], 3)[1]) and (got[3][:, 3:] == -1).all()
        assert same3(got, expected_from(s["M"], cells, got[3], k)), k
        assert same3(got, kq.expected(s["M"], k, SCALE)), k


# ---- 5. edges ----

def test_edges_and_repeatability():
    lib, ptr, check, ctx, st, d = tq._api()
    s = restricted_setup()
    p = s["p"]
    # no query row: nothing is written
    got = raw_ivf_q8(s["qf"][:0], s["q8"][:0], p, 8, 8)
    assert got[0].shape == (0, 8)
    # no database row: unfilled slots only
    empty = make_parts(np.zeros((0, 128), np.int8), np.zeros(0, np.int64), s["cent"])
    for nprobe in (1, 8):
        d2, dist, idx, probes = raw_ivf_q8(s["qf"], s["q8"], empty, 3, nprobe)
        assert (idx == -1).all() and np.isposinf(dist).all() and (d2 == kq.INT32_MAX).all() and (probes >= 0).all()
    # the same call twice: the grouping's atomics may order a group differently, the result cannot differ
    for k, nprobe in ((8, 5), (2, 8), (1, 1)):
        a, b = raw_ivf_q8(s["qf"], s["q8"], p, k, nprobe, (50, 60)), raw_ivf_q8(s["qf"], s["q8"], p, k, nprobe, (50, 60))
        assert same3(a, b) and same(a[3], b[3])
    # a refused call writes nothing
    buf = full((4096,), SENT_I32, torch.int32)
    b = ptr(buf)
    for bad in (dict(k=0), dict(k=9), dict(np=0), dict(np=9), dict(dim=64), dict(nc=0), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")),
                dict(scale=float("inf"))):
        a = dict(dict(k=8, np=8, dim=128, nc=len(SIZES), scale=SCALE), **bad)
        rc = lib.affnet_ivf_search_q8(ctx, b, b, b, 4, ptr(p["sorted_q"]), ptr(p["sorted_sq"]), ptr(p["perm"]), N2, ptr(p["cell_start"]), ptr(p["centroids"]),
                                      a["nc"], a["dim"], a["k"], a["np"], 0, 0, a["scale"], b, b, b, b, b, st)
        assert rc == -1 and b"ivf" in lib.affnet_last_error(ctx), bad
    torch.cuda.synchronize()
    assert (buf == SENT_I32).all()


# ---- 6. the Python layer ----

def test_parts_are_the_float_parts_with_quantised_rows():
    from affnet_amd import retrieval as R
    v = kf.vote_setup()
    D = dev(v["D"])
    cent = R.train_cells(D, 8)
    scale = R.quantization_scale(D)
    f, p = R.IVFParts(D, cent), R.IVFQ8Parts(D, cent, scale)
    assert p.n_cells == 8 and p.scale == scale and torch.equal(p.centroids, f.centroids)
    assert p.perm.dtype == torch.int32 and torch.equal(p.perm, f.perm) and torch.equal(p.cell_start, f.cell_start)
    perm = p.perm.cpu().numpy()
    want_q, want_sq = kq.quantize(v["D"], scale)
    assert p.sorted_q.dtype == torch.int8 and same(p.sorted_q.cpu().numpy(), want_q[perm])
    assert p.sorted_sq.dtype == torch.int32 and same(p.sorted_sq.cpu().numpy(), want_sq[perm])
    Dq, sq = R.quantize(D, scale)
    assert torch.equal(p.sorted_q, Dq[p.perm.long()]) and torch.equal(p.sorted_sq, sq[p.perm.long()])
    # the search alone, with its probes, against the restriction of the mirror's matrix
    q = v["queries"][3]
    d2, dist, idx, probes = [t.cpu().numpy() for t in R.ivf_knn_q8(dev(q), p, k=4, nprobe=2, return_probes=True)]
    assert same(probes, R.ivf_knn(dev(q), f, k=4, nprobe=2, return_probes=True)[2].cpu().numpy())
    cell_of_row = np.empty(perm.size, np.int64)
    cell_of_row[perm] = np.repeat(np.arange(8), np.diff(p.cell_start.cpu().numpy()))
    want = iq.expected(kq.quantize(q, scale)[0], want_q, cell_of_row, probes, 4, scale)
    assert same(d2, want[0]) and same(dist, want[1]) and same(idx, want[2])
    e = R.ivf_knn_q8(torch.zeros(0, 128, device=DEV), p, k=3)
    assert e[0].shape == e[1].shape == e[2].shape == (0, 3)


@pytest.mark.parametrize("n_cells", [1, 8])
def test_index_votes_equal_the_quantised_index(n_cells):
    from affnet_amd import retrieval as R
    v = kf.vote_setup()
    descs = [dev(d) for d in v["descs"]]
    q8 = R.QuantizedDescriptorIndex(descs)
    index = R.IVFQuantizedDescriptorIndex(descs, scale=q8.scale, n_cells=n_cells, nprobe=n_cells)
    lean = R.IVFQuantizedDescriptorIndex(descs, scale=q8.scale, n_cells=n_cells, nprobe=n_cells, keep_float=False)
    assert index.n_cells == n_cells == lean.n_cells and index.scale == q8.scale and index.D is not None and torch.equal(index.Dq, q8.Dq)
    assert lean.D is None and lean.Dq is None and lean.sq is None and lean.n_rows == q8.n_rows
    assert torch.equal(lean.ivf.sorted_q, index.ivf.sorted_q) and torch.equal(lean.ivf.perm, index.ivf.perm)
    rows = lean.n_rows
    held = sum(t.numel() * t.element_size() for t in (lean.ivf.sorted_q, lean.ivf.sorted_sq, lean.ivf.perm))
    assert held == 136 * rows, "136 bytes per row"
    for s in (1, 3, 5, 7):
        q = dev(v["queries"][s])
        for k, exclude in ((4, None), (8, None), (4, s), (2, 0)):
            want = q8.enqueue_votes(q, k=k, exclude=exclude)
            for ix in (index, lean):
                got = ix.enqueue_votes(q, k=k, exclude=exclude)
                for a, b in zip(got, want):
                    assert a.dtype == b.dtype and same(a.cpu().numpy(), b.cpu().numpy()), (s, k, exclude)
        assert index.shortlist(q) == lean.shortlist(q) == q8.shortlist(q) == ([s], [kf.VOTE_COUNTS[s]])
        assert lean.shortlist(q, exclude=s) == q8.shortlist(q, exclude=s)
    with pytest.raises(ValueError, match="keep_float=False"):
        lean.retrieve(dev(v["queries"][1]), torch.zeros(45, 2, 3, device=DEV))
    with pytest.raises(ValueError, match="without LAFs"):
        index.retrieve(dev(v["queries"][1]), torch.zeros(45, 2, 3, device=DEV))


def test_nprobe_is_an_attribute():
    from affnet_amd import retrieval as R
    v = kf.vote_setup()
    descs = [dev(d) for d in v["descs"]]
    index = R.IVFQuantizedDescriptorIndex(descs, n_cells=8, nprobe=1)
    q8 = R.QuantizedDescriptorIndex(descs, scale=index.scale)
    q = dev(v["queries"][5])
    one = index.enqueue_votes(q, k=4)
    alone = R.ivf_knn_q8(q, index, k=4, nprobe=1)
    assert torch.equal(one[1], alone[1]) and torch.equal(one[2], alone[2])
    index.nprobe = 8
    every, want = index.enqueue_votes(q, k=4), q8.enqueue_votes(q, k=4)
    assert all(torch.equal(a, b) for a, b in zip(every, want))
    assert not torch.equal(one[2], every[2]), "one cell of eight holds fewer of a row's four neighbours than all eight"
    index.nprobe = 9
    with pytest.raises(ValueError, match="nprobe must be"):
        index.enqueue_votes(q, k=4)


def test_retrieve_equals_match_and_verify():
    from affnet_amd import retrieval as R
    from affnet_amd import ReprojectionStuff as RS
    s = tq.image_set()
    descs, lafs = s["descs"], s["lafs"]
    q8 = R.QuantizedDescriptorIndex(descs, lafs)
    index = R.IVFQuantizedDescriptorIndex(descs, lafs, scale=q8.scale, n_cells=8, nprobe=8)
    assert torch.equal(index.D, q8.D) and torch.equal(index.L, q8.L)
    for query, exclude in ((7, None), (7, 7), (4, 4)):
        assert index.shortlist(descs[query], top=5, exclude=exclude) == q8.shortlist(descs[query], top=5, exclude=exclude)
        res, want = index.retrieve(descs[query], lafs[query], top=5, exclude=exclude), q8.retrieve(descs[query], lafs[query], top=5, exclude=exclude)
        assert len(want) >= 2 and [r["image"] for r in res] == [r["image"] for r in want]
        for r, w in zip(res, want):
            assert sorted(r) == sorted(w) and (r["votes"], r["num_inliers"]) == (w["votes"], w["num_inliers"])
            t1, t2, H, inl, info = RS.match_and_verify(descs[query], descs[r["image"]], lafs[query], lafs[r["image"]])
            assert torch.equal(r["tent_in_1"], t1) and torch.equal(r["tent_in_2"], t2) and same(r["H"].cpu().numpy(), H.cpu().numpy())
            assert torch.equal(r["inliers"], inl) and r["num_inliers"] == info["num_inliers"]
