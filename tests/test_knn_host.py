"""CPU: the host side of the descriptor index (csrc/knn.hip affnet_knn / affnet_knn_vote, affnet_amd/retrieval.py): the boundary's
declarations, the size helpers, the argument checks in front of the first launch, the index's bookkeeping, and the float64 restatement
(tests/_knn_fp64.py) that the GPU tests compare against, on hand-worked cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _knn_fp64 as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_four_functions():
    from affnet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "affnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    _P, _I = C.c_void_p, C.c_int
    want = {"affnet_knn_chunks": (_I, [_P, _I, _I]),
            "affnet_knn_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
            "affnet_knn": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
            "affnet_knn_vote": (_I, [_P, _P, _P, _I, _I, C.c_float, _P, _I, _I, _P, _P])}
    for name, (res, args) in want.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        declared = [a.strip() for a in m.group(1).split(",")]
        assert len(declared) == len(args), name
        for d, a in zip(declared, args):        # pointer / int / float, argument by argument
            kind = _P if "*" in d else (C.c_float if d.startswith("float") else _I)
            assert kind is a, (name, d)
        assert _lib.SYMBOLS[name] == (res, args), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define\s+AFFNET_KNN_MAX_K\s+8\b", hdr) and _lib.KNN_MAX_K == 8
    # the vote contract states what k - 1 bounds
    assert re.search(r"k - 1 is the largest number of database images that can show the same feature", raw)


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import retrieval
    assert affnet_amd.knn is retrieval.knn and affnet_amd.DescriptorIndex is retrieval.DescriptorIndex


def test_scratch_bytes():
    from affnet_amd import _lib
    f = _lib.lib.affnet_knn_scratch_bytes
    sizes = (0, 1, 15, 16, 17, 63, 64, 65, 200, 2000, 65536)
    for pos, values in ((0, sizes), (1, sizes), (2, range(0, 9)), (3, (1, 2, 3, 7, 30, 64, 1024))):
        for others in ((1, 1, 1, 1), (17, 415, 3, 7), (2000, 65536, 8, 32)):
            def at(v):
                a = list(others)
                a[pos] = v
                return f(*a)
            got = [at(v) for v in values]
            assert all(b >= a for a, b in zip(got, got[1:])), (pos, got)
    # room for the two norm vectors and the partial lists of every chunk
    for n1, n2, k, nc in ((1, 1, 1, 1), (130, 415, 8, 30), (2000, 1048576, 8, 32)):
        assert f(n1, n2, k, nc) >= 4 * (n1 + n2) + 8 * n1 * nc * k
    # n_chunks = 0: whatever the library may choose
    lib = _lib.lib
    for n1, n2 in ((1, 1), (64, 1048576), (2000, 2000), (2000, 1048576), (100000, 100000)):
        assert f(n1, n2, 8, 0) >= f(n1, n2, 8, lib.affnet_knn_chunks(None, n1, n2))
    assert f(0, 0, 0, 0) == f(0, 0, 0, 1) == f(0, 2000, 8, 0) - 4 * 2000, "no rows, no lists"
    assert f(-1, -1, -1, -1) == f(0, 0, 0, 1) and f(-5, 100, 3, 2) == f(0, 100, 3, 2), "negative arguments count as 0"


def test_chunks_choice():
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        for ctx in (None, h):
            for n1 in (0, 1, 64, 65, 2000, 1 << 20):
                got = [lib.affnet_knn_chunks(ctx, n1, n2) for n2 in (0, 1, 15, 16, 17, 415, 2000, 65536, 1 << 20, 0x7fffffff)]
                assert all(1 <= g <= 65535 for g in got), (n1, got)
                assert all(b >= a for a, b in zip(got, got[1:])), "a larger database never gets fewer chunks"
            assert lib.affnet_knn_chunks(ctx, -1, -1) >= 1
            assert lib.affnet_knn_chunks(ctx, 2000, 16) == 1, "one tile, one chunk"
            assert lib.affnet_knn_chunks(ctx, 64, 1 << 20) > lib.affnet_knn_chunks(ctx, 2000, 1 << 20) > 1, "fewer row blocks, more chunks"
    finally:
        lib.affnet_ctx_destroy(h)


CHUNK_N2 = (0, 1, 16, 79, 80, 415, 2000, 65536, 1 << 20, 2 ** 31 - 1)
# affnet_knn_chunks(NULL, n1, n2) over CHUNK_N2, recorded from the build before the chunk choice became one function shared with the int8 search
# (256 CUs, 3 workgroups per CU over cdiv(n1, 64) row blocks, no chunk below 5 tiles of 16 columns).  A slip there changes speed and no result byte.
KNN_CHUNKS = {
    1: (1, 1, 1, 1, 1, 5, 25, 768, 768, 768),
    64: (1, 1, 1, 1, 1, 5, 25, 768, 768, 768),
    65: (1, 1, 1, 1, 1, 5, 25, 384, 384, 384),
    256: (1, 1, 1, 1, 1, 5, 25, 192, 192, 192),
    257: (1, 1, 1, 1, 1, 5, 25, 154, 154, 154),
    2000: (1, 1, 1, 1, 1, 5, 24, 24, 24, 24),
    4000: (1, 1, 1, 1, 1, 5, 13, 13, 13, 13),
}


def test_chunks_table():
    from affnet_amd import _lib
    for n1, want in KNN_CHUNKS.items():
        assert tuple(_lib.lib.affnet_knn_chunks(None, n1, n2) for n2 in CHUNK_N2) == want, n1


def test_bad_arguments_are_refused_before_any_device_work():
    """The argument checks run on the host, in front of the first launch: they need no GPU, and no pointer below is ever dereferenced."""
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        p = C.c_void_p(4096)
        ok = dict(q=p, n1=4, db=p, n2=4, dim=128, k=2, row=0, n=0, nc=0, dist=p, idx=p, scr=p)

        def knn(**kw):
            a = dict(ok, **kw)
            return lib.affnet_knn(h, a["q"], a["n1"], a["db"], a["n2"], a["dim"], a["k"], a["row"], a["n"], a["nc"], a["dist"], a["idx"], a["scr"], None)
        for kw in (dict(k=0), dict(k=9), dict(k=-1), dict(dim=64), dict(n1=-1), dict(n2=-1), dict(n=-1), dict(nc=-1), dict(nc=65536), dict(q=None), dict(db=None),
                   dict(dist=None), dict(idx=None), dict(scr=None)):
            assert knn(**kw) == _lib.ERR_INVALID, kw
            assert b"knn" in lib.affnet_last_error(h), kw
        assert knn(n1=0) == _lib.OK, "no query row: valid, nothing is launched"
        okv = dict(dist=p, idx=p, n1=4, k=2, ratio=0.8, ri=p, n2=4, M=3, votes=p)

        def vote(**kw):
            a = dict(okv, **kw)
            return lib.affnet_knn_vote(h, a["dist"], a["idx"], a["n1"], a["k"], a["ratio"], a["ri"], a["n2"], a["M"], a["votes"], None)
        for kw in (dict(k=0), dict(k=9), dict(n1=-1), dict(n2=-1), dict(M=-1), dict(dist=None), dict(idx=None), dict(ri=None), dict(votes=None)):
            assert vote(**kw) == _lib.ERR_INVALID, kw
            assert b"knn_vote" in lib.affnet_last_error(h), kw
        assert vote(M=0) == _lib.OK, "no image: valid, nothing is launched"
    finally:
        lib.affnet_ctx_destroy(h)


def test_python_argument_errors_need_no_device():
    from affnet_amd import retrieval as R
    q, db = torch.zeros(3, 128), torch.zeros(5, 128)
    with pytest.raises(ValueError, match="device tensor"):
        R.knn(q, db)
    for k in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            R.knn(q, db, k=k)
    with pytest.raises(ValueError):
        R.knn(torch.zeros(3, 64), db)
    with pytest.raises(ValueError, match="device tensor"):
        R.DescriptorIndex([db, q])
    with pytest.raises(ValueError, match="one LAF per descriptor row"):
        R.DescriptorIndex([db, q], [torch.zeros(5, 2, 3), torch.zeros(4, 2, 3)])
    with pytest.raises(ValueError, match="one LAF tensor per descriptor tensor"):
        R.DescriptorIndex([db, q], [torch.zeros(5, 2, 3)])
    with pytest.raises(ValueError):
        R.DescriptorIndex([])
    for bad in (4, -1, 1.0):
        with pytest.raises(ValueError, match="exclude"):
            R.skip_range([5, 0, 17, 3], bad)
    # an index without frames cannot retrieve (the check stands in front of everything else; the object below never touches a device)
    idx = object.__new__(R.DescriptorIndex)
    idx.L, idx.counts = None, [5]
    with pytest.raises(ValueError, match="without LAFs"):
        idx.retrieve(q, torch.zeros(3, 2, 3))


def test_index_bookkeeping():
    from affnet_amd import retrieval as R
    counts, off = R.index_offsets([5, 0, 17, 3])          # ragged, image 1 is empty
    assert counts == [5, 0, 17, 3] and off == [0, 5, 5, 22, 25]
    assert [R.skip_range(counts, e) for e in (None, 0, 1, 2, 3)] == [(0, 0), (0, 5), (5, 0), (5, 17), (22, 3)]
    assert R.index_offsets([]) == ([], [0])
    with pytest.raises(ValueError):
        R.index_offsets([3, -1])
    with pytest.raises(ValueError):
        R.index_offsets([1 << 30, 1 << 30, 1])
    idx = object.__new__(R.DescriptorIndex)          # the methods of the class read the same tables
    idx.counts, idx.offsets = counts, off
    assert len(idx) == 4 and idx.skip_range(2) == (5, 17) and idx.skip_range(None) == (0, 0)


def test_fp64_distance_and_order():
    a = np.array([[1.0, 0.0], [0.0, 2.0]])
    b = np.array([[1.0, 0.0], [0.0, 0.0], [3.0, 4.0]])
    d = kf.distance(a, b)
    want = np.sqrt(np.array([[0.0, 1.0, 20.0], [5.0, 4.0, 13.0]]) + 1e-6)
    assert np.allclose(d, want, rtol=0, atol=1e-12)
    # (NaN first, distance, index): ties by index, several NaNs by index
    row = np.array([0.5, np.nan, 0.25, 0.5, np.nan, 0.25, np.inf])
    assert kf.order(row).tolist() == [1, 4, 2, 5, 0, 3, 6]
    M = np.array([row, [3.0, 2.0, 1.0, 1.0, 2.0, 3.0, 0.5]], np.float32)
    dist, idx = kf.sorted_knn(M, 3)
    assert idx.tolist() == [[1, 4, 2], [6, 2, 3]] and dist.dtype == np.float32
    assert np.isnan(dist[0, :2]).all() and dist[0, 2] == 0.25 and dist[1].tolist() == [0.5, 1.0, 1.0]
    # skip range: inside, clipped at both ends, everything
    assert kf.sorted_knn(M, 3, (1, 4))[1].tolist() == [[5, 0, 6], [6, 0, 5]]
    assert kf.sorted_knn(M, 2, (-3, 5))[1].tolist() == [[4, 2], [6, 2]]
    assert kf.sorted_knn(M, 2, (5, 100))[1].tolist() == [[1, 4], [2, 3]]
    dist, idx = kf.sorted_knn(M, 2, (0, 7))
    assert (idx == -1).all() and np.isposinf(dist).all()
    # fewer candidates than k: unfilled slots
    dist, idx = kf.sorted_knn(M[:, :2], 4)
    assert idx.tolist() == [[1, 0, -1, -1], [1, 0, -1, -1]] and np.isposinf(dist[:, 2:]).all()
    dist, idx = kf.sorted_knn(np.zeros((2, 0), np.float32), 3)
    assert idx.shape == (2, 3) and (idx == -1).all() and np.isposinf(dist).all()


def test_fp64_vote_rule():
    row_image = np.array([0, 0, 1, 1, 2, 2])
    # row 0: neighbour 0 stands out, neighbour 1 does not (0.9 > 0.8 * 1.0); row 1: two neighbours in image 1, one vote; row 2: unfilled last slot,
    # every real neighbour votes; row 3: a NaN votes, a tie with the bound votes (not greater)
    dist = np.array([[0.1, 0.9, 1.0], [0.1, 0.2, 1.0], [0.5, 0.7, np.inf], [np.nan, 0.8, 1.0]])
    idx = np.array([[0, 2, 4], [2, 3, 4], [1, 5, -1], [4, 0, 2]])
    assert kf.votes(dist, idx, 0.8, row_image, 3).tolist() == [3, 1, 2]
    assert kf.votes(dist[:1], idx[:1], 0.8, row_image, 3).tolist() == [1, 0, 0]
    assert kf.votes(dist[1:2], idx[1:2], 0.8, row_image, 3).tolist() == [0, 1, 0]
    assert kf.votes(dist[2:3], idx[2:3], 0.8, row_image, 3).tolist() == [1, 0, 1]
    assert kf.votes(dist[3:], idx[3:], 0.8, row_image, 3).tolist() == [1, 0, 1]
    # the last slot itself never votes; k = 1 gives zeros
    assert kf.votes(dist[:, :1], idx[:, :1], 0.8, row_image, 3).tolist() == [0, 0, 0]
    assert kf.votes(np.array([[0.1, 0.2]]), np.array([[0, 2]]), 0.8, row_image, 3).tolist() == [1, 0, 0]
    # ids out of range are skipped: a row beyond the table, an image beyond n_images, a negative id other than -1
    assert kf.votes(np.array([[0.1, 0.1, 0.1, 1.0]]), np.array([[6, -2, 4, 0]]), 0.8, row_image, 2).tolist() == [0, 0]
    # margin: the closest comparison is |0.8 - 0.8 * 1.0| = 0
    assert kf.vote_margin(dist[:2], idx[:2], 0.8) == pytest.approx(0.1) and kf.vote_margin(dist[3:], idx[3:], 0.8) == pytest.approx(0.0)
    assert kf.vote_margin(dist[:, :1], idx[:, :1], 0.8) == np.inf


@pytest.mark.parametrize("k", [2, 3, 8])
def test_fp64_votes_on_the_test_images(k):
    """The setup of the GPU vote test, decided in float64: the query's source image gets one vote per descriptor and nobody else any, every
    comparison of the rule has a wide margin, and leaving the source image out leaves no vote at all."""
    v = kf.vote_setup()
    M = len(kf.VOTE_COUNTS)
    for s in (1, 3, 5, 7):
        D = kf.distance(v["queries"][s], v["D"])
        dist, idx = kf.sorted_knn(D, k)
        assert kf.vote_margin(dist, idx, 0.8) > 0.079
        want = np.zeros(M, np.int32)
        want[s] = kf.VOTE_COUNTS[s]
        assert kf.votes(dist, idx, 0.8, v["row_image"], M).tolist() == want.tolist()
        dist, idx = kf.sorted_knn(D, k, (int(v["off"][s]), kf.VOTE_COUNTS[s]))
        assert kf.vote_margin(dist, idx, 0.8) > 0.079
        assert not kf.votes(dist, idx, 0.8, v["row_image"], M).any()
    if k == 8:      # without the ratio gate the largest image wins
        D = kf.distance(v["queries"][1], v["D"])
        dist, idx = kf.sorted_knn(D, k)
        plain = np.bincount(v["row_image"][idx[:, :k - 1]].ravel(), minlength=M)
        assert plain.argmax() == M - 1


def test_fp64_votes_for_two_copies():
    """Two database images that are noisy copies of the same source: with k = 3 both receive every vote (k - 1 = 2 images can share a feature)."""
    v = kf.vote_setup()
    D = kf.distance(v["queries"][3], np.concatenate([v["D"], v["twin"]]))
    row_image = np.concatenate([v["row_image"], np.full(len(v["twin"]), 9, np.int32)])
    dist, idx = kf.sorted_knn(D, 3)
    assert kf.vote_margin(dist, idx, 0.8) > 0.079
    got = kf.votes(dist, idx, 0.8, row_image, 10)
    assert got[3] == got[9] == kf.VOTE_COUNTS[3] and got.sum() == 2 * kf.VOTE_COUNTS[3]
