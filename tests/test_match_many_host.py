"""CPU: the host side of matching and verifying many image pairs per device call (csrc/match.hip affnet_match_snn_many, csrc/spatial.hip
affnet_verify_matches_many, ReprojectionStuff.pair_table / match_and_verify_many / spatial_rerank): the pair table, the scratch sizes, the
argument checks in front of the first launch, and the boundary's declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_table():
    from affnet_amd import ReprojectionStuff as RS
    counts = [5, 0, 17, 3]          # ragged, image 1 is empty
    table, n1_max, n2_max = RS.pair_table(counts, counts, [(0, 2), (0, 3), (0, 0), (1, 2), (3, 1), (2, 2)])      # image 0 is a repeated query
    assert table.dtype == np.int32 and table.shape == (6, 4)
    assert table.tolist() == [[0, 5, 5, 17], [0, 5, 22, 3], [0, 5, 0, 5], [5, 0, 5, 17], [22, 3, 5, 0], [5, 17, 5, 17]]
    assert (n1_max, n2_max) == (17, 17)
    # two different sides
    table, n1_max, n2_max = RS.pair_table([4, 6], [1, 2, 3], [(1, 0), (0, 2), (1, 1)])
    assert table.tolist() == [[4, 6, 0, 1], [0, 4, 3, 3], [4, 6, 1, 2]] and (n1_max, n2_max) == (6, 3)
    # no pair
    table, n1_max, n2_max = RS.pair_table(counts, counts, [])
    assert table.shape == (0, 4) and table.dtype == np.int32 and (n1_max, n2_max) == (0, 0)
    for bad in ([(0, 4)], [(4, 0)], [(-1, 0)], [(0, 1), (0, -1)]):
        with pytest.raises(ValueError):
            RS.pair_table(counts, counts, bad)
    with pytest.raises(ValueError):
        RS.pair_table([3, -1], [3], [(0, 0)])


def test_scratch_sizes():
    from affnet_amd import _lib
    lib = _lib.lib
    sizes = (0, 1, 15, 16, 17, 63, 64, 65, 200, 2000)
    # monotone in each argument
    for f, nargs in ((lib.affnet_match_many_scratch_bytes, 3), (lib.affnet_verify_many_scratch_bytes, 2)):
        for k in range(nargs):
            for others in ((1, 1), (3, 17), (32, 2000)):
                def at(v):
                    a = list(others[:nargs - 1])
                    a.insert(k, v)
                    return f(*a)
                got = [at(v) for v in sizes]
                assert all(b >= a for a, b in zip(got, got[1:])), (f.__name__, k, got)
    # at least P x the data part of the single-pair size (what that call adds for alignment is its trailing 64 bytes), 0-safe
    for P in (0, 1, 2, 32):
        for n1, n2 in ((1, 1), (17, 200), (2000, 2000), (64, 1)):
            assert lib.affnet_match_many_scratch_bytes(P, n1, n2) >= P * (lib.affnet_match_scratch_bytes(n1, n2) - 64)
            assert lib.affnet_verify_many_scratch_bytes(P, n1) >= P * (lib.affnet_verify_scratch_bytes(n1) - 64)
    assert lib.affnet_match_many_scratch_bytes(0, 2000, 2000) >= 0 and lib.affnet_verify_many_scratch_bytes(0, 2000) >= 0
    assert lib.affnet_match_many_scratch_bytes(0, 0, 0) == lib.affnet_match_many_scratch_bytes(0, 2000, 2000), "no pair, no data"
    assert lib.affnet_match_many_scratch_bytes(-1, -1, -1) == lib.affnet_match_many_scratch_bytes(0, 0, 0), "negative arguments count as 0"
    assert lib.affnet_verify_many_scratch_bytes(-1, -1) == lib.affnet_verify_many_scratch_bytes(0, 0)


def test_header_declares_and_lib_binds_the_four_functions():
    from affnet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "affnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in (("affnet_match_many_scratch_bytes", 3), ("affnet_match_snn_many", 18), ("affnet_verify_many_scratch_bytes", 2),
                        ("affnet_verify_matches_many", 19)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    # flag 8 = pair row out of range: defined, documented, and the value Python uses
    assert re.search(r"#define\s+AFFNET_VERIFY_FLAG_PAIR_RANGE\s+8\b", hdr) and _lib.VERIFY_FLAG_PAIR_RANGE == 8
    assert re.search(r"AFFNET_VERIFY_FLAG_PAIR_RANGE 8\s*/\*[^*]*pair row out of range", raw)


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import ReprojectionStuff as RS
    for name in ("pair_table", "enqueue_match_and_verify_many", "match_and_verify_many", "spatial_rerank"):
        assert getattr(affnet_amd, name) is getattr(RS, name)
    with pytest.raises(RuntimeError):
        RS.match_and_verify_many([np.zeros((1, 128))], [np.zeros((1, 2, 3))], [(0, 0)])        # no CPU path
    assert RS.match_and_verify_many([], [], []) == []


def test_bad_arguments_are_refused_before_any_device_work():
    """The argument checks run on the host, in front of the first launch: they need no GPU, and no pointer below is ever dereferenced."""
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        p = C.c_void_p(4096)
        ok = dict(d1=p, r1=8, d2=p, r2=8, dim=128, pairs=p, P=2, n1=4, n2=4, md=p, idx=p, md2=p, tent=p, cnt=p, scr=p)

        def snn(**kw):
            a = dict(ok, **kw)
            return lib.affnet_match_snn_many(h, a["d1"], a["r1"], a["d2"], a["r2"], a["dim"], a["pairs"], a["P"], a["n1"], a["n2"], 0.8, a["md"], a["idx"], a["md2"],
                                             a["tent"], a["cnt"], a["scr"], None)
        for kw in (dict(dim=64), dict(pairs=None), dict(n1=-1), dict(n2=-1), dict(P=-1), dict(r1=-1), dict(r2=-1), dict(d1=None), dict(d2=None), dict(md=None),
                   dict(idx=None), dict(md2=None), dict(tent=None), dict(cnt=None), dict(scr=None), dict(P=65536)):
            assert snn(**kw) == _lib.ERR_INVALID, kw
            assert b"match_snn_many" in lib.affnet_last_error(h), kw
        assert snn(P=0) == _lib.OK, "no pair: valid, nothing is launched"
        okv = dict(l1=p, r1=8, l2=p, r2=8, pairs=p, P=2, tent=p, count=None, t=4, th=3.0, model=1, it=3, counts=p, H=p, inl=p, summ=p, scr=p)

        def ver(**kw):
            a = dict(okv, **kw)
            return lib.affnet_verify_matches_many(h, a["l1"], a["r1"], a["l2"], a["r2"], a["pairs"], a["P"], a["tent"], a["count"], a["t"], a["th"], a["model"],
                                                  a["it"], a["counts"], a["H"], a["inl"], a["summ"], a["scr"], None)
        for kw in (dict(pairs=None), dict(t=-1), dict(P=-1), dict(r1=-1), dict(r2=-1), dict(l1=None), dict(l2=None), dict(tent=None), dict(counts=None),
                   dict(H=None), dict(inl=None), dict(summ=None), dict(scr=None), dict(scr=C.c_void_p(4100)), dict(th=0.0), dict(th=float("nan")), dict(model=2),
                   dict(it=9), dict(it=-1), dict(P=65536)):
            assert ver(**kw) == _lib.ERR_INVALID, kw
            assert b"verify_matches_many" in lib.affnet_last_error(h), kw
        assert ver(P=0) == _lib.OK and ver(P=0, count=p) == _lib.OK
    finally:
        lib.affnet_ctx_destroy(h)
