"""CPU: the host side of the inverted-file search over int8 rows (csrc/ivf.hip affnet_ivf_search_q8, affnet_amd/retrieval.py): the boundary's
declarations, the scratch size, the argument checks in front of the first launch, the Python argument errors, and the restatement
(tests/_ivf_q8.py) that the GPU tests compare against."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _ivf_q8 as iq
import _knn_q8 as kq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_two_functions():
    from affnet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "affnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    _P, _I, _F = C.c_void_p, C.c_int, C.c_float
    want = {"affnet_ivf_q8_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
            "affnet_ivf_search_q8": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P])}
    for name, (res, args) in want.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        declared = [a.strip() for a in m.group(1).split(",")]
        assert len(declared) == len(args), name
        for d, a in zip(declared, args):        # pointer / float / int, argument by argument
            assert (_P if "*" in d else (_F if d.startswith("float") else _I)) is a, (name, d)
        assert _lib.SYMBOLS[name] == (res, args), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    names = [a.strip().split()[-1].lstrip("*") for a in re.search(r"\baffnet_ivf_search_q8\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert names == ["ctx", "d_q", "d_qq", "d_qsq", "n1", "d_sorted_q", "d_sorted_sq", "d_perm", "n2", "d_cell_start", "d_centroids", "n_cells", "dim",
                     "k", "nprobe", "skip_row", "skip_n", "scale", "d_dist2", "d_dist", "d_idx", "d_probes", "d_scratch", "stream"]


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import retrieval
    for name in ("ivf_knn_q8", "IVFQ8Parts", "IVFQuantizedDescriptorIndex"):
        assert getattr(affnet_amd, name) is getattr(retrieval, name)
    assert issubclass(retrieval.IVFQuantizedDescriptorIndex, retrieval.QuantizedDescriptorIndex)
    own = set(vars(retrieval.IVFQuantizedDescriptorIndex)) - {"__doc__", "__module__"}
    assert own == {"__init__", "_search"}, "enqueue_votes, shortlist, retrieve and its keep_float guard are inherited: the class replaces the search alone"


def test_scratch_bytes():
    from affnet_amd import _lib
    f = _lib.lib.affnet_ivf_q8_scratch_bytes
    sizes = (0, 1, 15, 16, 17, 63, 64, 65, 200, 2000, 65536)
    for pos, values in ((0, sizes), (1, sizes), (2, range(0, 9)), (3, range(0, 9))):
        for others in ((1, 1, 1, 1), (17, 11, 3, 7), (2000, 1024, 8, 8)):
            def at(v):
                a = list(others)
                a[pos] = v
                return f(*a)
            got = [at(v) for v in values]
            assert all(b >= a for a, b in zip(got, got[1:])), (pos, got)
    # room for the coarse step, the pairs and their groups, the work items and the partial lists (int32 d2 and rows)
    for n1, nc, p, k in ((1, 1, 1, 1), (130, 11, 8, 8), (2000, 1024, 8, 2)):
        items = -(-n1 * p // 16) + min(nc, n1 * p)
        assert f(n1, nc, p, k) >= _lib.lib.affnet_knn_scratch_bytes(n1, nc, p, _lib.lib.affnet_knn_chunks(None, n1, nc)) + \
            3 * 4 * n1 * p + 3 * 4 * nc + 8 * items + 8 * n1 * p * k
    assert f(2000, 1024, 8, 8) < 1 << 24, "the operating point needs a few megabytes"
    assert f(0, 0, 0, 0) > 0 and f(-1, -1, -1, -1) == f(0, 0, 0, 0) and f(-5, 100, 3, 2) == f(0, 100, 3, 2), "negative arguments count as 0"


def test_bad_arguments_are_refused_before_any_device_work():
    """The argument checks run on the host, in front of the first launch: they need no GPU, and no pointer below is ever dereferenced."""
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        p = C.c_void_p(4096)
        ok = dict(q=p, qq=p, qsq=p, n1=4, srt=p, ssq=p, perm=p, n2=4, cs=p, cen=p, nc=2, dim=128, k=2, np=2, row=0, n=0, scale=100.0, d2=p, dist=p,
                  idx=p, probes=p, scr=p)

        def search(**kw):
            a = dict(ok, **kw)
            return lib.affnet_ivf_search_q8(h, a["q"], a["qq"], a["qsq"], a["n1"], a["srt"], a["ssq"], a["perm"], a["n2"], a["cs"], a["cen"], a["nc"],
                                            a["dim"], a["k"], a["np"], a["row"], a["n"], a["scale"], a["d2"], a["dist"], a["idx"], a["probes"], a["scr"], None)
        for kw in (dict(dim=64), dict(k=0), dict(k=9), dict(k=-1), dict(np=0), dict(np=9), dict(np=-1), dict(nc=0), dict(nc=-3), dict(n1=-1), dict(n2=-1),
                   dict(n=-1), dict(n1=1 << 30), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
                   dict(q=None), dict(qq=None), dict(qsq=None), dict(srt=None), dict(ssq=None), dict(perm=None), dict(cs=None), dict(cen=None),
                   dict(d2=None), dict(dist=None), dict(idx=None), dict(scr=None)):
            assert search(**kw) == _lib.ERR_INVALID, kw
            assert b"ivf" in lib.affnet_last_error(h), kw
        assert search(n1=0) == _lib.OK, "no query row: valid, nothing is launched"
        assert search(n1=0, probes=None) == _lib.OK, "the probes are an optional output"
    finally:
        lib.affnet_ctx_destroy(h)


def test_python_argument_errors_need_no_device():
    from affnet_amd import retrieval as R
    q, db = torch.zeros(3, 128), torch.zeros(5, 128)
    parts = object.__new__(R.IVFQ8Parts)
    for k in (0, 9, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            R.ivf_knn_q8(q, parts, k=k)
    for nprobe in (0, 9, -1, 1.5):
        with pytest.raises(ValueError, match="nprobe must be"):
            R.ivf_knn_q8(q, parts, nprobe=nprobe)
        with pytest.raises(ValueError, match="nprobe must be"):
            R.IVFQuantizedDescriptorIndex([db], nprobe=nprobe)
    for other in (db, object.__new__(R.IVFParts)):
        with pytest.raises(ValueError, match="IVFQuantizedDescriptorIndex or IVFQ8Parts"):
            R.ivf_knn_q8(q, other)
    with pytest.raises(ValueError, match="device tensor"):
        R.ivf_knn_q8(q, parts)
    for n_cells in (0, -1, 2.0):
        with pytest.raises(ValueError, match="n_cells"):
            R.IVFQuantizedDescriptorIndex([db], n_cells=n_cells)
    with pytest.raises(ValueError, match="device tensor"):
        R.IVFQuantizedDescriptorIndex([db, q])
    for scale in (0.0, -2.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="scale must be"):
            R.IVFQ8Parts(db, db, scale)
    with pytest.raises(ValueError, match="device tensor"):
        R.IVFQ8Parts(db, db, 100.0)


def test_restricted_knn_int_with_all_cells_probed_is_sorted_knn_int():
    rng = np.random.default_rng(11)
    M = rng.integers(0, 50, size=(9, 40)).astype(np.int64)          # 40 columns over 50 values: ties in every row
    M[2, 5] = M[2, 17] = M[2, 30] = -1                               # planted below every other value: the row decides
    M[3, :] = 7                                                      # one value everywhere: the order is the rows'
    assert all(len(set(row.tolist())) < 40 for row in M)
    cells = rng.integers(0, 5, 40)
    every = np.tile(np.arange(5), (9, 1))
    for k in (1, 3, 8):
        for skip in ((0, 0), (4, 10), (-3, 8), (35, 100), (0, 40)):
            want, got = kq.sorted_knn_int(M, k, skip), iq.restricted_knn_int(M, cells, every, k, skip)
            assert got[0].dtype == want[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, skip)
    assert iq.restricted_knn_int(M, cells, every, 3)[1][2].tolist() == [5, 17, 30] and iq.restricted_knn_int(M, cells, every, 3)[1][3].tolist() == [0, 1, 2]
    # a restriction: only the probed cells' columns, -1 names no cell
    probes = np.array([[1, -1]] * 9)
    d, i = iq.restricted_knn_int(M, cells, probes, 8)
    n = int((cells == 1).sum())
    assert ((i == -1) | (cells[np.maximum(i, 0)] == 1)).all() and (i[:, :min(n, 8)] >= 0).all()
    if n < 8:
        assert (i[:, n:] == -1).all() and (d[:, n:] == kq.INT32_MAX).all()
    d, i = iq.restricted_knn_int(M, cells, np.full((9, 2), -1), 3)
    assert (i == -1).all() and (d == kq.INT32_MAX).all()
    # the three outputs from two int8 arrays: the float distance is fdist of the d2, +inf where there is no candidate
    qa, qb = kq.random_rows(9, 1), kq.random_rows(40, 2)
    d2, dist, idx = iq.expected(qa, qb, cells, probes, 8, 335.07)
    full = kq.dist2(qa, qb)
    assert dist.dtype == np.float32 and np.isposinf(dist[idx < 0]).all()
    assert (d2[idx >= 0] == np.take_along_axis(full, np.maximum(idx, 0).astype(np.int64), 1)[idx >= 0]).all()
    assert np.array_equal(dist[idx >= 0], kq.fdist(d2[idx >= 0], 335.07))
