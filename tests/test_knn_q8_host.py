"""CPU: the host side of the int8 descriptor index (csrc/knn_q8.hip affnet_quantize_desc / affnet_knn_q8, affnet_amd/retrieval.py): the
boundary's declarations, the size helpers, the argument checks in front of the first launch, the Python argument errors, and the numpy mirror
(tests/_knn_q8.py) that the GPU tests compare against - its own properties on the vote fixture of tests/_knn_fp64.py and the error bound of the
reported distance."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _knn_fp64 as kf
import _knn_q8 as kq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_four_functions():
    from affnet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "affnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    _P, _I, _F = C.c_void_p, C.c_int, C.c_float
    want = {"affnet_quantize_desc": (_I, [_P, _P, _I, _I, _F, _P, _P, _P]),
            "affnet_knn_q8_chunks": (_I, [_P, _I, _I]),
            "affnet_knn_q8_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I]),
            "affnet_knn_q8": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P])}
    for name, (res, args) in want.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        declared = [a.strip() for a in m.group(1).split(",")]
        assert len(declared) == len(args), name
        for d, a in zip(declared, args):        # pointer / int / float, argument by argument
            kind = _P if "*" in d else (_F if d.startswith("float") else _I)
            assert kind is a, (name, d)
        assert _lib.SYMBOLS[name] == (res, args), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    # the contract states the rule, the order and the bound
    assert "clamp(rintf(x * scale), -127, 127)" in raw and "the smaller d2, then the smaller database row" in raw and "sqrt(128) / scale" in raw


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import retrieval as R
    assert affnet_amd.quantization_scale is R.quantization_scale and affnet_amd.quantize is R.quantize and affnet_amd.knn_q8 is R.knn_q8
    assert affnet_amd.QuantizedDescriptorIndex is R.QuantizedDescriptorIndex and issubclass(R.QuantizedDescriptorIndex, R.DescriptorIndex)
    assert R.QuantizedDescriptorIndex.shortlist is R.DescriptorIndex.shortlist, "shortlist is inherited"


def test_scratch_bytes():
    from affnet_amd import _lib
    f = _lib.lib.affnet_knn_q8_scratch_bytes
    sizes = (0, 1, 15, 16, 17, 63, 64, 65, 200, 2000, 65536)
    for pos, values in ((0, sizes), (1, sizes), (2, range(0, 9)), (3, (1, 2, 3, 7, 30, 64, 1024))):
        for others in ((1, 1, 1, 1), (17, 415, 3, 7), (2000, 65536, 8, 32)):
            def at(v):
                a = list(others)
                a[pos] = v
                return f(*a)
            got = [at(v) for v in values]
            assert all(b >= a for a, b in zip(got, got[1:])), (pos, got)
    # room for the partial lists of every chunk: one int32 d2 and one int32 row per slot
    for n1, n2, k, nc in ((1, 1, 1, 1), (130, 415, 8, 30), (2000, 1048576, 8, 32)):
        assert f(n1, n2, k, nc) >= 8 * n1 * nc * k
    # n_chunks = 0: whatever the library may choose
    lib = _lib.lib
    for n1, n2 in ((1, 1), (64, 1048576), (2000, 2000), (2000, 1048576), (100000, 100000)):
        assert f(n1, n2, 8, 0) >= f(n1, n2, 8, lib.affnet_knn_q8_chunks(None, n1, n2))
    assert f(0, 0, 0, 0) == f(0, 0, 0, 1) == f(0, 2000, 8, 0), "no rows, no lists"
    assert f(-1, -1, -1, -1) == f(0, 0, 0, 1) and f(-5, 100, 3, 2) == f(0, 100, 3, 2), "negative arguments count as 0"


def test_chunks_choice():
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        for ctx in (None, h):
            for n1 in (0, 1, 64, 65, 128, 129, 256, 257, 2000, 1 << 20):
                got = [lib.affnet_knn_q8_chunks(ctx, n1, n2) for n2 in (0, 1, 31, 32, 33, 415, 2000, 65536, 1 << 20, 0x7fffffff)]
                assert all(1 <= g <= 65535 for g in got), (n1, got)
                assert all(b >= a for a, b in zip(got, got[1:])), "a larger database never gets fewer chunks"
            assert lib.affnet_knn_q8_chunks(ctx, -1, -1) >= 1
            assert lib.affnet_knn_q8_chunks(ctx, 2000, 32) == 1, "one step, one chunk"
            assert lib.affnet_knn_q8_chunks(ctx, 64, 1 << 20) > lib.affnet_knn_q8_chunks(ctx, 2000, 1 << 20) > 1, "fewer row blocks, more chunks"
    finally:
        lib.affnet_ctx_destroy(h)


CHUNK_N2 = (0, 1, 16, 79, 80, 415, 2000, 65536, 1 << 20, 2 ** 31 - 1)
# affnet_knn_q8_chunks(NULL, n1, n2) over CHUNK_N2, recorded from the build before the chunk choice became one function shared with the fp32
# search (256 CUs, 2 workgroups per CU over cdiv(n1, 256) row blocks, no chunk below 2 steps of 32 columns).  The second table is
# affnet_knn_q8_chunks(NULL, 2 n1, n2): the choice for the 128-row blocks of k > 2 (tools/knn_q8_rate.py).  A slip changes speed and no result byte.
Q8_CHUNKS = {
    1: (1, 1, 1, 1, 1, 6, 31, 512, 512, 512),
    64: (1, 1, 1, 1, 1, 6, 31, 512, 512, 512),
    65: (1, 1, 1, 1, 1, 6, 31, 512, 512, 512),
    256: (1, 1, 1, 1, 1, 6, 31, 512, 512, 512),
    257: (1, 1, 1, 1, 1, 6, 31, 256, 256, 256),
    2000: (1, 1, 1, 1, 1, 6, 31, 64, 64, 64),
    4000: (1, 1, 1, 1, 1, 6, 31, 32, 32, 32),
}
Q8_CHUNKS_128 = {
    1: (1, 1, 1, 1, 1, 6, 31, 512, 512, 512),
    64: (1, 1, 1, 1, 1, 6, 31, 512, 512, 512),
    65: (1, 1, 1, 1, 1, 6, 31, 512, 512, 512),
    256: (1, 1, 1, 1, 1, 6, 31, 256, 256, 256),
    257: (1, 1, 1, 1, 1, 6, 31, 171, 171, 171),
    2000: (1, 1, 1, 1, 1, 6, 31, 32, 32, 32),
    4000: (1, 1, 1, 1, 1, 6, 16, 16, 16, 16),
}


def test_chunks_table():
    from affnet_amd import _lib
    f = _lib.lib.affnet_knn_q8_chunks
    for n1, want in Q8_CHUNKS.items():
        assert tuple(f(None, n1, n2) for n2 in CHUNK_N2) == want, n1
    for n1, want in Q8_CHUNKS_128.items():
        assert tuple(f(None, 2 * n1, n2) for n2 in CHUNK_N2) == want, n1


BAD_SCALES = (0.0, -1.0, float("nan"), float("inf"))


def test_bad_arguments_are_refused_before_any_device_work():
    """The argument checks run on the host, in front of the first launch: they need no GPU, and no pointer below is ever dereferenced."""
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        p = C.c_void_p(4096)
        ok = dict(q=p, qsq=p, n1=4, db=p, dbsq=p, n2=4, dim=128, k=2, row=0, n=0, nc=0, scale=300.0, d2=p, dist=p, idx=p, scr=p)

        def knn(**kw):
            a = dict(ok, **kw)
            return lib.affnet_knn_q8(h, a["q"], a["qsq"], a["n1"], a["db"], a["dbsq"], a["n2"], a["dim"], a["k"], a["row"], a["n"], a["nc"], a["scale"],
                                     a["d2"], a["dist"], a["idx"], a["scr"], None)
        bad = [dict(k=0), dict(k=9), dict(k=-1), dict(dim=64), dict(n1=-1), dict(n2=-1), dict(n=-1), dict(nc=-1), dict(nc=65536), dict(q=None), dict(qsq=None),
               dict(db=None), dict(dbsq=None), dict(d2=None), dict(dist=None), dict(idx=None), dict(scr=None)] + [dict(scale=s) for s in BAD_SCALES]
        for kw in bad:
            assert knn(**kw) == _lib.ERR_INVALID, kw
            assert b"knn_q8" in lib.affnet_last_error(h), kw
        assert knn(n1=0) == _lib.OK, "no query row: valid, nothing is launched"
        okq = dict(desc=p, n=4, dim=128, scale=300.0, q=p, sq=p)

        def quant(**kw):
            a = dict(okq, **kw)
            return lib.affnet_quantize_desc(h, a["desc"], a["n"], a["dim"], a["scale"], a["q"], a["sq"], None)
        for kw in [dict(n=-1), dict(dim=64), dict(dim=0), dict(desc=None), dict(q=None), dict(sq=None)] + [dict(scale=s) for s in BAD_SCALES]:
            assert quant(**kw) == _lib.ERR_INVALID, kw
            assert b"quantize_desc" in lib.affnet_last_error(h), kw
        assert quant(n=0) == _lib.OK, "no row: a no-op"
    finally:
        lib.affnet_ctx_destroy(h)


def test_python_argument_errors_need_no_device():
    from affnet_amd import retrieval as R
    x = torch.zeros(3, 128)
    q, sq = torch.zeros(3, 128, dtype=torch.int8), torch.zeros(3, dtype=torch.int32)
    db, dbsq = torch.zeros(5, 128, dtype=torch.int8), torch.zeros(5, dtype=torch.int32)
    for s in BAD_SCALES + (None, "x", 1e39):
        with pytest.raises(ValueError, match="scale"):
            R.quantize(x, s)
        with pytest.raises(ValueError, match="scale"):
            R.knn_q8(q, sq, db, dbsq, scale=s)
    with pytest.raises(ValueError, match="device tensor"):
        R.quantize(x, 300.0)
    with pytest.raises(ValueError):
        R.quantize(torch.zeros(3, 64), 300.0)
    with pytest.raises(ValueError, match="device tensor"):
        R.knn_q8(q, sq, db, dbsq, scale=300.0)
    for k in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            R.knn_q8(q, sq, db, dbsq, k=k, scale=300.0)
    with pytest.raises(ValueError, match="int8"):
        R.knn_q8(x, sq, db, dbsq, scale=300.0)
    with pytest.raises(ValueError, match="int8"):
        R.knn_q8(q, sq, torch.zeros(5, 64, dtype=torch.int8), dbsq, scale=300.0)
    with pytest.raises(ValueError, match="sum of squares"):
        R.knn_q8(q, dbsq, db, dbsq, scale=300.0)
    with pytest.raises(ValueError, match="sum of squares"):
        R.knn_q8(q, sq.float(), db, dbsq, scale=300.0)
    with pytest.raises(ValueError, match="no finite non-zero entry"):
        R.quantization_scale([x, torch.zeros(0, 128)])
    with pytest.raises(ValueError, match="device tensor"):
        R.QuantizedDescriptorIndex([x])
    with pytest.raises(ValueError):
        R.QuantizedDescriptorIndex([])
    assert R.quantization_scale(torch.tensor([[0.25, -0.5]])) == 254.0 and R.quantization_scale([torch.tensor([[0.25]]), torch.tensor([[-0.5]])]) == 254.0
    # an index without float descriptors cannot retrieve (the check stands in front of everything else; the object below never touches a device)
    idx = object.__new__(R.QuantizedDescriptorIndex)
    idx.D, idx.L, idx.counts = None, torch.zeros(5, 2, 3), [5]
    with pytest.raises(ValueError, match="keep_float=False"):
        idx.retrieve(x, torch.zeros(3, 2, 3))


def test_mirror_on_hand_worked_cases():
    x = np.zeros((2, 128), np.float32)
    x[0, :8] = [0.25, 0.75, 1.25, 1.75, -0.25, -0.75, -1.25, 63.75]          # exact halves at scale 2: to the even neighbour
    x[1, :6] = [np.nan, np.inf, -np.inf, 100.0, -100.0, 63.5]
    q, sq = kq.quantize(x, 2.0)
    assert q.dtype == np.int8 and sq.dtype == np.int32
    assert q[0, :8].tolist() == [0, 2, 2, 4, 0, -2, -2, 127] and q[1, :6].tolist() == [0, 127, -127, 127, -127, 127] and not q[:, 8:].any()
    assert sq.tolist() == [4 + 4 + 16 + 4 + 4 + 127 * 127, 5 * 127 * 127]
    a = np.array([[127] * 128, [3] + [0] * 127, [0] * 128], np.int8)
    b = np.array([[-127] * 128, [0, 4] + [0] * 126, [3] + [0] * 127], np.int8)
    M = kq.dist2(a, b)
    assert M.dtype == np.int64 and M[0, 0] == kq.D2_MAX == 8258048 and M[1].tolist() == [128 * 127 * 127 + 2 * 3 * 127 + 9, 25, 0]
    assert kq.fdist(np.array([25, 0, kq.D2_MAX]), 2.0).tolist() == [2.5, 0.0, float(np.sqrt(np.float32(8258048)) / np.float32(2))]
    # (d2, row): ties by row; skip range clipped at both ends; unfilled slots
    M = np.array([[5, 3, 5, 3, 9], [0, 0, 0, 0, 0]])
    assert kq.sorted_knn_int(M, 3)[1].tolist() == [[1, 3, 0], [0, 1, 2]] and kq.sorted_knn_int(M, 3)[0].tolist() == [[3, 3, 5], [0, 0, 0]]
    assert kq.sorted_knn_int(M, 2, (1, 2))[1].tolist() == [[3, 0], [0, 3]]
    assert kq.sorted_knn_int(M, 2, (-3, 5))[1].tolist() == [[3, 2], [2, 3]]
    assert kq.sorted_knn_int(M, 2, (3, 100))[1].tolist() == [[1, 0], [0, 1]]
    d2, idx = kq.sorted_knn_int(M, 2, (0, 5))
    assert (idx == -1).all() and (d2 == kq.INT32_MAX).all() and d2.dtype == idx.dtype == np.int32
    d2, dist, idx = kq.expected(M[:, :2], 4, 2.0)
    assert idx.tolist() == [[1, 0, -1, -1], [0, 1, -1, -1]] and (d2[:, 2:] == kq.INT32_MAX).all() and np.isposinf(dist[:, 2:]).all()
    assert dist.dtype == np.float32 and dist[1, :2].tolist() == [0.0, 0.0]
    d2, dist, idx = kq.expected(np.zeros((2, 0), np.int64), 3, 2.0)
    assert idx.shape == (2, 3) and (idx == -1).all() and np.isposinf(dist).all()


_VQ = {}


def vote_q8():
    """The vote fixture of tests/_knn_fp64.py quantised with scale = float32(127 / max|D|), made once."""
    if not _VQ:
        v = kf.vote_setup()
        scale = float(np.float32(127.0 / float(np.abs(v["D"]).max())))
        Dq, _ = kq.quantize(v["D"], scale)
        _VQ.update(v=v, scale=scale, Dq=Dq, Q={s: kq.quantize(v["queries"][s], scale)[0] for s in (1, 3, 5, 7)})
    return _VQ


def test_mirror_properties_on_the_vote_fixture():
    f = vote_q8()
    v, scale = f["v"], f["scale"]
    assert abs(scale - 335.07) < 0.01
    M = len(kf.VOTE_COUNTS)
    worst = 0.0
    for s in (1, 3, 5, 7):
        q = v["queries"][s]
        assert np.abs(q * np.float32(scale)).max() <= 127.0, "no query entry is clipped"
        d2 = kq.dist2(f["Q"][s], f["Dq"])
        assert d2.min() >= 0 and d2.max() < 2 ** 24
        D64 = kf.distance(q, v["D"])
        fd = kq.fdist(d2, scale)
        worst = max(worst, float(np.abs(fd.astype(np.float64) - D64).max()))
        # the bound, not a fitted number: each of the two rows moves by at most 0.5 sqrt(128) / scale in the 2-norm, the triangle inequality
        # does the rest, and the 1e-6 under the reference's root moves a distance by at most 1e-3
        assert np.abs(fd.astype(np.float64) - D64).max() <= np.sqrt(128.0) / scale + 1e-3
        n = kf.VOTE_COUNTS[s]
        w_d, w_i = kf.sorted_knn(D64, 8)
        g_d2, g_i = kq.sorted_knn_int(d2, 8)
        assert (g_i[:n, 0] == w_i[:n, 0]).all(), "the quantised nearest neighbour is the float64 one on every planted row"
        assert (np.diff(g_d2.astype(np.int64), axis=1) > 0).all(), "no row has a tie among its first 8"
        want = np.zeros(M, np.int32)
        want[s] = n
        for k in (2, 4, 8):
            g_d2, g_i = kq.sorted_knn_int(d2, k)
            w_d, w_i = kf.sorted_knn(D64, k)
            got = kf.votes(kq.fdist(g_d2, scale), g_i, np.float32(0.8), v["row_image"], M, np.float32)
            assert got.tolist() == kf.votes(w_d, w_i, 0.8, v["row_image"], M).tolist() == want.tolist(), (s, k)
    print("max |fdist - float64 distance| = %.4f (bound %.4f)" % (worst, np.sqrt(128.0) / scale + 1e-3))
    assert abs(worst - 0.0057) < 0.0005, "the figure the documents quote"
