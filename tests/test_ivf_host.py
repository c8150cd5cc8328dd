"""CPU: the host side of the inverted-file search (csrc/ivf.hip, affnet_amd/retrieval.py): the boundary's declarations, the scratch size, the
argument checks in front of the first launch, the cell layout on CPU tensors, the Python argument errors, and the restatement
(tests/_ivf.py) that the GPU tests compare against."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _ivf as iv
import _knn_fp64 as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_four_functions():
    from affnet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "affnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    _P, _I = C.c_void_p, C.c_int
    want = {"affnet_ivf_sqnorm": (_I, [_P, _P, _I, _I, _P, _P]),
            "affnet_ivf_cell_means": (_I, [_P, _P, _I, _I, _P, _P, _I, _P, _P]),
            "affnet_ivf_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
            "affnet_ivf_search": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P])}
    for name, (res, args) in want.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        declared = [a.strip() for a in m.group(1).split(",")]
        assert len(declared) == len(args), name
        for d, a in zip(declared, args):        # pointer / int, argument by argument
            assert (_P if "*" in d else _I) is a, (name, d)
        assert _lib.SYMBOLS[name] == (res, args), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define\s+AFFNET_IVF_MAX_PROBE\s+8\b", hdr) and _lib.IVF_MAX_PROBE == 8 == _lib.KNN_MAX_K


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import retrieval
    for name in ("train_cells", "ivf_layout", "ivf_knn", "IVFDescriptorIndex"):
        assert getattr(affnet_amd, name) is getattr(retrieval, name)
    assert issubclass(retrieval.IVFDescriptorIndex, retrieval.DescriptorIndex)
    own = set(vars(retrieval.IVFDescriptorIndex)) - {"__init__", "__doc__", "__module__"}
    assert own == {"_search"}, "enqueue_votes, shortlist and retrieve are inherited: the class replaces the search alone"


def test_scratch_bytes():
    from affnet_amd import _lib
    f = _lib.lib.affnet_ivf_scratch_bytes
    sizes = (0, 1, 15, 16, 17, 63, 64, 65, 200, 2000, 65536)
    for pos, values in ((0, sizes), (1, sizes), (2, range(0, 9)), (3, range(0, 9))):
        for others in ((1, 1, 1, 1), (17, 11, 3, 7), (2000, 1024, 8, 8)):
            def at(v):
                a = list(others)
                a[pos] = v
                return f(*a)
            got = [at(v) for v in values]
            assert all(b >= a for a, b in zip(got, got[1:])), (pos, got)
    # room for the coarse step, the pairs and their groups, the work items and the partial lists
    for n1, nc, p, k in ((1, 1, 1, 1), (130, 11, 8, 8), (2000, 1024, 8, 2)):
        items = -(-n1 * p // 16) + min(nc, n1 * p)
        assert f(n1, nc, p, k) >= _lib.lib.affnet_knn_scratch_bytes(n1, nc, p, _lib.lib.affnet_knn_chunks(None, n1, nc)) + \
            4 * n1 + 3 * 4 * n1 * p + 3 * 4 * nc + 8 * items + 8 * n1 * p * k
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
        ok = dict(q=p, n1=4, srt=p, ssq=p, perm=p, n2=4, cs=p, cen=p, nc=2, dim=128, k=2, np=2, row=0, n=0, dist=p, idx=p, probes=p, scr=p)

        def search(**kw):
            a = dict(ok, **kw)
            return lib.affnet_ivf_search(h, a["q"], a["n1"], a["srt"], a["ssq"], a["perm"], a["n2"], a["cs"], a["cen"], a["nc"], a["dim"], a["k"],
                                         a["np"], a["row"], a["n"], a["dist"], a["idx"], a["probes"], a["scr"], None)
        for kw in (dict(dim=64), dict(k=0), dict(k=9), dict(k=-1), dict(np=0), dict(np=9), dict(np=-1), dict(nc=0), dict(nc=-3), dict(n1=-1), dict(n2=-1),
                   dict(n=-1), dict(q=None), dict(srt=None), dict(ssq=None), dict(perm=None), dict(cs=None), dict(cen=None), dict(dist=None),
                   dict(idx=None), dict(scr=None), dict(n1=1 << 30)):
            assert search(**kw) == _lib.ERR_INVALID, kw
            assert b"ivf" in lib.affnet_last_error(h), kw
        assert search(n1=0) == _lib.OK, "no query row: valid, nothing is launched"
        assert search(n1=0, probes=None) == _lib.OK, "the probes are an optional output"

        def sqnorm(**kw):
            a = dict(dict(x=p, n=4, dim=128, out=p), **kw)
            return lib.affnet_ivf_sqnorm(h, a["x"], a["n"], a["dim"], a["out"], None)
        for kw in (dict(dim=64), dict(n=-1), dict(x=None), dict(out=None)):
            assert sqnorm(**kw) == _lib.ERR_INVALID, kw
            assert b"ivf" in lib.affnet_last_error(h), kw
        assert sqnorm(n=0) == _lib.OK

        def means(**kw):
            a = dict(dict(x=p, n=4, dim=128, perm=p, cs=p, nc=2, cen=p), **kw)
            return lib.affnet_ivf_cell_means(h, a["x"], a["n"], a["dim"], a["perm"], a["cs"], a["nc"], a["cen"], None)
        for kw in (dict(dim=64), dict(n=-1), dict(nc=0), dict(x=None), dict(perm=None), dict(cs=None), dict(cen=None)):
            assert means(**kw) == _lib.ERR_INVALID, kw
            assert b"ivf" in lib.affnet_last_error(h), kw
        assert means(n=0) == _lib.OK
    finally:
        lib.affnet_ctx_destroy(h)


def test_ivf_layout_on_cpu_tensors():
    from affnet_amd import retrieval as R
    assign = torch.tensor([2, 0, 2, 4, 0, 2, 4, 4, 4], dtype=torch.int32)          # cells 1 and 3 are empty
    perm, start = R.ivf_layout(assign, 6)
    assert perm.dtype == torch.int32 and start.dtype == torch.int32
    assert perm.tolist() == [1, 4, 0, 2, 5, 3, 6, 7, 8], "stable: ascending inside every cell"
    assert start.tolist() == [0, 2, 2, 5, 5, 9, 9] and int(start[-1]) == assign.numel()
    rng = np.random.default_rng(5)
    for n, nc in ((0, 1), (1, 1), (1, 3), (415, 11), (1000, 3)):
        a = rng.integers(0, nc, n)
        perm, start = R.ivf_layout(torch.from_numpy(a), nc)
        want = iv.layout(a, nc)
        assert perm.tolist() == want[0].tolist() and start.tolist() == want[1].tolist() and int(start[-1]) == n
        for c in range(nc):
            seg = perm[int(start[c]):int(start[c + 1])].tolist()
            assert seg == sorted(seg) and all(a[r] == c for r in seg)
    for bad in (torch.tensor([0, 3]), torch.tensor([-1, 0])):
        with pytest.raises(ValueError, match="cell outside"):
            R.ivf_layout(bad, 3)
    with pytest.raises(ValueError):
        R.ivf_layout(torch.zeros(3), 3)
    with pytest.raises(ValueError):
        R.ivf_layout(torch.zeros(3, dtype=torch.int64), 0)


def test_python_argument_errors_need_no_device():
    from affnet_amd import retrieval as R
    q, db = torch.zeros(3, 128), torch.zeros(5, 128)
    parts = object.__new__(R.IVFParts)
    for k in (0, 9, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            R.ivf_knn(q, parts, k=k)
    for nprobe in (0, 9, -1, 1.5):
        with pytest.raises(ValueError, match="nprobe must be"):
            R.ivf_knn(q, parts, nprobe=nprobe)
        with pytest.raises(ValueError, match="nprobe must be"):
            R.IVFDescriptorIndex([db], nprobe=nprobe)
    with pytest.raises(ValueError, match="IVFDescriptorIndex or IVFParts"):
        R.ivf_knn(q, db)
    with pytest.raises(ValueError, match="device tensor"):
        R.ivf_knn(q, parts)
    with pytest.raises(ValueError, match="device tensor"):
        R.train_cells(db, 2)
    for n_cells in (0, -1, 2.0):
        with pytest.raises(ValueError, match="n_cells"):
            R.train_cells(db, n_cells)
        with pytest.raises(ValueError, match="n_cells"):
            R.IVFDescriptorIndex([db], n_cells=n_cells)
    with pytest.raises(ValueError, match="iters"):
        R.train_cells(db, 2, iters=-1)
    with pytest.raises(ValueError, match="device tensor"):
        R.IVFDescriptorIndex([db, q])
    assert [R.default_cells(n) for n in (0, 1, 4, 49, 65536, 1 << 20, 10 ** 7)] == [1, 1, 2, 8, 256, 1024, 4096]
    assert R.initial_cells(10, 4) == iv.initial_rows(10, 4) == [0, 2, 5, 7] and R.initial_cells(2, 4) == [0, 0, 1, 1]


def test_restricted_knn_with_all_cells_probed_is_sorted_knn():
    rng = np.random.default_rng(11)
    M = rng.random((9, 40)).astype(np.float32)
    M[2, 5] = M[2, 17] = M[2, 30] = 0.0          # ties: the row decides
    M[3, 8] = M[3, 33] = np.nan                    # NaNs stand in front
    cells = rng.integers(0, 5, 40)
    every = np.tile(np.arange(5), (9, 1))
    for k in (1, 3, 8):
        for skip in ((0, 0), (4, 10), (-3, 8), (35, 100), (0, 40)):
            want, got = kf.sorted_knn(M, k, skip), iv.restricted_knn(M, cells, every, k, skip)
            assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes(), (k, skip)
    # a restriction: only the probed cells' columns, -1 names no cell
    probes = np.array([[1, -1]] * 9)
    d, i = iv.restricted_knn(M, cells, probes, 8)
    n = int((cells == 1).sum())
    assert n < 8 or (i >= 0).all()
    assert ((i == -1) | (cells[np.maximum(i, 0)] == 1)).all() and (i[:, :min(n, 8)] >= 0).all()
    if n < 8:
        assert (i[:, n:] == -1).all() and np.isposinf(d[:, n:]).all()
    d, i = iv.restricted_knn(M, cells, np.full((9, 2), -1), 3)
    assert (i == -1).all() and np.isposinf(d).all()


def test_fp64_lloyd_step():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [10.0, 0.0], [11.0, 0.0], [12.0, 0.0]])
    c = x[iv.initial_rows(5, 2)]          # rows 0 and 2
    assert iv.assign(x, c).tolist() == [0, 0, 1, 1, 1]
    c1 = iv.lloyd_step(x, c)
    assert c1.tolist() == [[0.5, 0.0], [11.0, 0.0]] and iv.objective(x, c1) == pytest.approx(2.5) and iv.objective(x, c) == pytest.approx(6.0)
    # an empty cell keeps its centroid; ties go to the smaller cell
    c = np.array([[0.0, 0.0], [0.0, 0.0], [100.0, 0.0]])
    assert iv.assign(x, c).tolist() == [0] * 5
    assert iv.lloyd_step(x, c).tolist() == [[6.8, 0.0], [0.0, 0.0], [100.0, 0.0]]
