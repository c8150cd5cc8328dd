"""CPU: the many-pairs forms of the epipolar verification and of guided matching (affnet_epipolar_verify_many, affnet_match_guided_many and the
Python functions over them) are part of the boundary, size their scratch sensibly and refuse bad arguments on the host, in front of any launch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = (("affnet_epipolar_many_scratch_bytes", 3), ("affnet_epipolar_verify_many", 20), ("affnet_match_guided_many_scratch_bytes", 4),
       ("affnet_match_guided_many", 26))


def test_header_declares_and_lib_binds_the_entry_points():
    from affnet_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "affnet_hip.h")).read(), flags=re.S)
    for name, nargs in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name + " is not declared in include/affnet_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)


def test_python_names_are_exported():
    import affnet_amd
    from affnet_amd import ReprojectionStuff as RS
    for name in ("enqueue_match_verify_guided_many", "match_verify_guided_many", "enqueue_match_and_verify_many", "match_and_verify_many", "spatial_rerank"):
        assert getattr(affnet_amd, name) is getattr(RS, name)


def test_epipolar_scratch_bytes():
    from affnet_amd import _lib
    f, one = _lib.lib.affnet_epipolar_many_scratch_bytes, _lib.lib.affnet_epipolar_scratch_bytes
    Ps, ts, rs = (0, 1, 2, 3, 32, 1000, 65535), (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 2000), (1, 2, 3, 8, 63, 64)
    for P in Ps:
        for t in ts:
            for r in rs:
                assert f(P, t, r) >= P * (one(t, r) - 64), (P, t, r)
    mono = lambda v: all(b >= a for a, b in zip(v, v[1:]))
    for t in ts:
        for r in rs:
            assert mono([f(P, t, r) for P in Ps]), (t, r)
    for P in Ps:
        for r in rs:
            assert mono([f(P, t, r) for t in ts]), (P, r)
        for t in ts:
            assert mono([f(P, t, r) for r in range(0, 65)]), (P, t)
    assert f(1, 1, 1) > 0
    assert f(0, 0, 0) == f(-3, 100, 8) == f(0, 100, 8) and f(4, -1, 8) == f(4, 0, 8) and f(4, 100, -2) == f(4, 100, 0)


def test_guided_scratch_bytes():
    from affnet_amd import _lib
    f, one = _lib.lib.affnet_match_guided_many_scratch_bytes, _lib.lib.affnet_match_guided_scratch_bytes
    Ps, ns, cs = (0, 1, 2, 3, 32, 1000, 65535), (0, 1, 15, 16, 17, 63, 64, 65, 200, 2000), (0, 1, 2, 3, 7, 64)
    for P in Ps:
        for a in ns:
            for b in ns:
                for c in cs:
                    assert f(P, a, b, c) >= P * (one(a, b, c) - 64), (P, a, b, c)
    mono = lambda v: all(y >= x for x, y in zip(v, v[1:]))
    for a in ns:
        for b in ns:
            for c in cs:
                assert mono([f(P, a, b, c) for P in Ps]), (a, b, c)
    for P in Ps:
        for c in cs:
            for b in ns:
                assert mono([f(P, a, b, c) for a in ns]), (P, b, c)
            for a in ns:
                assert mono([f(P, a, b, c) for b in ns]), (P, a, c)
        for a in ns:
            for b in ns:
                # explicit chunk counts: more chunks, more partial lists; 0 = "the library chooses" is sized for the most it may choose
                assert mono([f(P, a, b, c) for c in range(1, 66)]), (P, a, b)
                assert f(P, a, b, 0) >= f(P, a, b, 1), (P, a, b)
    assert f(1, 1, 1, 1) > 0
    assert f(0, 0, 0, 0) == f(-3, 100, 100, 2) == f(0, 100, 100, 2)
    assert f(4, -1, 50, 2) == f(4, 0, 50, 2) and f(4, 50, -1, 2) == f(4, 50, 0, 2)
    assert f(4, 50, 50, -1) <= f(4, 50, 50, 1), "a negative chunk count counts as no partial list at all"


def test_models_and_rounds_are_checked_on_the_host():
    from affnet_amd import ReprojectionStuff as RS
    assert RS.match_and_verify_many([], [], [], model="fundamental") == []
    assert RS.match_and_verify_many([], [], []) == []
    assert RS.match_verify_guided_many([], [], [], model="fundamental") == []
    assert RS.spatial_rerank([], [], 0, [], model="fundamental", guided=True) == ([], [])
    with pytest.raises(ValueError):
        RS.match_and_verify_many([], [], [], model="essential")
    with pytest.raises(ValueError):
        RS.match_verify_guided_many([], [], [], model="essential")
    for rounds in (0, -1, 65):
        with pytest.raises(ValueError):
            RS.match_and_verify_many([], [], [], model="fundamental", rounds=rounds)
        with pytest.raises(ValueError):
            RS.match_verify_guided_many([], [], [], model="fundamental", rounds=rounds)
    assert RS.match_and_verify_many([], [], [], model="fundamental", rounds=1) == RS.match_and_verify_many([], [], [], model="fundamental", rounds=64) == []
    with pytest.raises(ValueError):
        RS.match_and_verify_many([], [], [], model="fundamental", seed=2 ** 32)


def test_bad_arguments_are_refused_before_any_device_work():
    """The argument checks run on the host, in front of the first launch: they need no GPU."""
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        p = C.c_void_p(4096)            # never dereferenced: every call below is refused, or has no pair
        nan, inf = float("nan"), float("inf")
        ok = dict(l1=p, rows1=40, l2=p, rows2=40, pairs=p, P=2, tent=p, count=None, t=4, th=2.0, rounds=8, seed=0, it=3, counts=p, F=p, inl=p, summ=p, scr=p)

        def verify(**kw):
            a = dict(ok, **kw)
            return lib.affnet_epipolar_verify_many(h, a["l1"], a["rows1"], a["l2"], a["rows2"], a["pairs"], a["P"], a["tent"], a["count"], a["t"], a["th"],
                                                   a["rounds"], a["seed"], a["it"], a["counts"], a["F"], a["inl"], a["summ"], a["scr"], None)
        bad = [dict(l1=None), dict(l2=None), dict(pairs=None), dict(tent=None), dict(counts=None), dict(F=None), dict(inl=None), dict(summ=None), dict(scr=None),
               dict(rows1=-1), dict(rows2=-1), dict(P=-1), dict(P=65536), dict(t=-1), dict(th=0.0), dict(th=-1.0), dict(th=nan), dict(th=inf), dict(rounds=0),
               dict(rounds=-1), dict(rounds=65), dict(it=-1), dict(it=9), dict(scr=C.c_void_p(4100)), dict(t=2 ** 31 - 1, rounds=2), dict(t=2 ** 26, rounds=32)]
        for kw in bad:
            assert verify(**kw) == _lib.ERR_INVALID, kw
            assert b"epipolar_verify_many" in lib.affnet_last_error(h), kw
        assert verify(P=0) == _lib.OK
        assert lib.affnet_epipolar_verify_many(None, p, 40, p, 40, p, 2, p, None, 4, 2.0, 8, 0, 3, p, p, p, p, p, None) == _lib.ERR_INVALID

        gk = dict(d1=p, rows1=40, d2=p, rows2=40, dim=128, l1=p, l2=p, pairs=p, P=2, n1=20, n2=20, model=p, kind=_lib.GUIDED_PLANAR, r=10.0, thr=0.9, md=inf,
                  flags=_lib.GUIDED_MUTUAL, nc=0, gate=None, dist=p, idx=p, tent=p, count=p, scr=p)

        def guided(**kw):
            a = dict(gk, **kw)
            return lib.affnet_match_guided_many(h, a["d1"], a["rows1"], a["d2"], a["rows2"], a["dim"], a["l1"], a["l2"], a["pairs"], a["P"], a["n1"], a["n2"],
                                                a["model"], a["kind"], a["r"], a["thr"], a["md"], a["flags"], a["nc"], a["gate"], a["dist"], a["idx"], a["tent"],
                                                a["count"], a["scr"], None)
        bad = [dict(d1=None), dict(d2=None), dict(l1=None), dict(l2=None), dict(pairs=None), dict(model=None), dict(dist=None), dict(idx=None), dict(tent=None),
               dict(count=None), dict(scr=None), dict(rows1=-1), dict(rows2=-1), dict(P=-1), dict(P=65536), dict(n1=-1), dict(n2=-1), dict(dim=64), dict(kind=2),
               dict(kind=-1), dict(flags=2), dict(r=0.0), dict(r=-1.0), dict(r=nan), dict(r=inf), dict(md=nan), dict(nc=-1), dict(nc=65536),
               dict(scr=C.c_void_p(4100))]
        for kw in bad:
            assert guided(**kw) == _lib.ERR_INVALID, kw
            assert b"match_guided_many" in lib.affnet_last_error(h), kw
        assert guided(P=0) == _lib.OK
        assert guided(P=0, gate=p, kind=_lib.GUIDED_EPIPOLAR, flags=0, nc=3) == _lib.OK
        assert lib.affnet_match_guided_many(None, p, 40, p, 40, 128, p, p, p, 2, 20, 20, p, 0, 10.0, 0.9, inf, 1, 0, None, p, p, p, p, p, None) == _lib.ERR_INVALID
    finally:
        lib.affnet_ctx_destroy(h)
