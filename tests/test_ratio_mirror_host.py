"""tests/_ratio_fp32.py, the float32 restatement of affnet_match_ratio, tied to what the project already trusts (the guided restatement's
first_k, a plain double loop) and to the properties of the rule; the scenes of tests/test_gpu_ratio_match.py proven to hold the cases they
claim; and the host side of the boundary: the scratch sizes and the argument checks that run in front of any launch.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import _guided_fp32 as gf
import _match_fp32 as mf
import _ratio_fp32 as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SHAPES = [(1, 1), (1, 17), (17, 33), (65, 200)]
RADII = (-1.0, 0.0, 3.0, 10.0, 25.0, 1e30)


def _scene(n1, n2):
    sc = rf.planted_scene(n1, n2)
    return sc, rf.scene_distance(("planted", n1, n2), sc)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_without_a_radius_the_slots_are_the_first_two_of_the_row(n1, n2):
    sc, M = _scene(n1, n2)
    got = rf.ratio_from(M, sc["l2"], -1.0, 0.8)
    d, i = gf.first_k(M, np.ones(M.shape, bool), 2)
    assert _same(got["dist"], d) and _same(got["idx"], i)
    got = rf.ratio_from(M, None, -1.0, 0.8)
    assert _same(got["dist"], d) and _same(got["idx"], i), "no frames are read without a radius"


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_slots_equal_a_plain_double_loop(n1, n2):
    sc, M = _scene(n1, n2)
    d1, i1 = gf.first_k(M, np.ones(M.shape, bool), 1)
    for r in RADII:
        got = rf.ratio_from(M, sc["l2"], r, 0.8)
        d, i = rf.ratio_loops(M, sc["l2"], r)
        assert _same(got["dist"], d) and _same(got["idx"], i), r
        assert _same(got["dist"][:, :1], d1) and _same(got["idx"][:, :1], i1), "slot 0 does not depend on the radius"
    if n2 > 1:
        assert (rf.ratio_from(M, sc["l2"], 1e30, 0.8)["idx"][:, 1] == -1).all(), "nothing is inconsistent at a radius that covers the window"


@pytest.mark.parametrize("n1,n2", SHAPES[1:])
def test_kept_sets_grow_with_the_radius(n1, n2):
    """The second distance at radius r is a minimum over a subset of the columns of every smaller radius, so it is no smaller, the ratio no
    larger, and what a smaller radius keeps a larger one keeps too (a NaN second distance comes first in the order at every radius)."""
    sc, M = _scene(n1, n2)
    for mutual in (False, True):
        kept = [rf.ratio_from(M, sc["l2"], r, 0.8, mutual=mutual)["keep"] for r in RADII]
        for small, large in zip(kept, kept[1:]):
            assert not (small & ~large).any()
        assert n1 < 17 or (kept[0].any() and not kept[0].all())
        assert not (kept[0] & ~kept[3]).any()
    sets = [rf.ratio_from(M, sc["l2"], r, 0.8)["keep"].sum() for r in RADII]
    if n2 >= 40:
        assert sets[3] > sets[0], "the planted scene has rows that only the radius lets through"


def test_radius_zero_differs_from_no_radius_on_the_planted_scene():
    sc, M = _scene(65, 200)
    a, b = rf.ratio_from(M, sc["l2"], -1.0, 0.8), rf.ratio_from(M, sc["l2"], 0.0, 0.8)
    assert (a["idx"][:, 1] != b["idx"][:, 1]).any(), "columns on exactly one place"
    u, v = gf.centres(sc["l2"])
    assert (u[21], v[21]) == (u[5], v[5]) and (u[11], v[11]) == (u[10], v[10])
    assert abs(np.hypot(u[38] - u[7], v[38] - v[7]) - 5.0) < 1e-4
    c = rf.ratio_from(M, sc["l2"], 10.0, 0.8)
    assert tuple(a["idx"][0]) == (5, 21) and b["idx"][0, 1] != 21, "row 0 copies columns 5 = 21"
    assert tuple(b["idx"][7]) == (7, 38) and c["idx"][7, 1] != 38, "row 7 copies columns 7 = 38"


def test_mutual_and_max_dist():
    sc, M = _scene(65, 200)
    plain, mutual = rf.ratio_from(M, sc["l2"], 10.0, 0.8), rf.ratio_from(M, sc["l2"], 10.0, 0.8, mutual=True)
    assert not (mutual["keep"] & ~plain["keep"]).any() and mutual["count"] < plain["count"], "several rows copy one pool row"
    for i, j in mutual["tent"]:
        assert mutual["back"][j] == i
    back = gf.first_k(M.T, np.ones(M.T.shape, bool), 1)[1][:, 0]
    assert (mutual["back"] == back).all()
    near = rf.ratio_from(M, sc["l2"], 10.0, 0.8, max_dist=0.5)
    assert 0 < near["count"] < plain["count"] and (near["dist"][near["keep"], 0] <= F32(0.5)).all()


# ---- the scenes hold what they claim ----------------------------------------------------------------------------------------------------
def _special(name):
    sc = rf.SPECIAL[name]()
    return sc, rf.scene_distance(name, sc)


def test_scene_a_twins_starve_the_plain_ratio_and_not_fginn():
    sc, M = _special("twin")
    plain, fginn = rf.ratio_from(M, sc["l2"], -1.0, 0.8), rf.ratio_from(M, sc["l2"], 10.0, 0.8)
    rows = sc["planted"]
    assert len(rows) == rf.TWINS
    assert not plain["keep"][rows].any() and fginn["keep"][rows].all()
    for i in rows:
        assert {int(plain["idx"][i, 0]), int(plain["idx"][i, 1])} == {i, rf.TWINS + i}, "partner and twin are the two nearest"
        assert fginn["idx"][i, 0] in (i, rf.TWINS + i) and fginn["idx"][i, 1] not in (i, rf.TWINS + i)
    u, v = gf.centres(sc["l2"])
    gap = np.hypot(u[:rf.TWINS] - u[rf.TWINS:2 * rf.TWINS], v[:rf.TWINS] - v[rf.TWINS:2 * rf.TWINS])
    assert np.allclose(gap, 1.5, atol=1e-3)


def test_scene_b_nine_columns_on_the_nearest_ones_place():
    sc, M = _special("nine")
    order = gf.first_k(M[:1], np.ones((1, M.shape[1]), bool), 11)[1][0]
    assert sorted(order[:10]) == list(range(20, 30)) and order[10] == 45
    inc = rf.inconsistent(sc["l2"], order[:1], 10.0)[0]
    assert not inc[20:30].any() and inc[45]
    got = rf.ratio_from(M, sc["l2"], 10.0, 0.8)
    assert tuple(got["idx"][0]) == (order[0], 45) and got["keep"][0]
    assert not rf.ratio_from(M, sc["l2"], -1.0, 0.8)["keep"][0]


def test_scene_c_a_column_exactly_on_the_radius_is_consistent():
    sc, M = _special("boundary")
    u, v = gf.centres(sc["l2"])
    assert (u[0], v[0], u[1], v[1], u[2]) == (100, 100, 106, 108, 106) and v[2] == np.nextafter(F32(108), F32(109))
    assert tuple(gf.first_k(M, np.ones(M.shape, bool), 3)[1][0]) == (0, 1, 2)
    inc = rf.inconsistent(sc["l2"], np.array([0]), 10.0)[0]
    assert not inc[1] and inc[2]
    assert tuple(rf.ratio_from(M, sc["l2"], 10.0, 0.8)["idx"][0]) == (0, 2)
    assert tuple(rf.ratio_from(M, sc["l2"], -1.0, 0.8)["idx"][0]) == (0, 1)


def test_scene_d_of_duplicate_rows_the_smaller_column_wins():
    sc, M = _special("duplicate")
    assert M[0, 3] == M[0, 7] and M[1, 10] == M[1, 12] and M[2, 19] == M[2, 35]
    for r in (-1.0, 10.0):
        got = rf.ratio_from(M, sc["l2"], r, 0.8)
        assert tuple(got["idx"][0]) == (3, 7) and not got["keep"][0]
        assert tuple(got["idx"][1]) == (9, 10)
        assert tuple(got["idx"][2]) == (19, 35)


def test_scene_e_no_inconsistent_column_keeps_the_row_with_ratio_zero():
    sc, M = _special("crowded")
    got = rf.ratio_from(M, sc["l2"], 10.0, 0.8)
    assert (got["idx"][:, 1] == -1).all() and np.isinf(got["dist"][:, 1]).all() and (got["ratio"] == 0).all() and got["keep"].all()
    assert got["idx"][0, 0] == 4
    assert (rf.ratio_from(M, sc["l2"], -1.0, 0.8)["idx"][:, 1] >= 0).all()


def test_scene_f_a_nan_nearest_distance_is_refused():
    sc, M = _special("nan")
    assert np.isnan(M[1, 6]) and np.isnan(M[1]).sum() == 1
    for r in (-1.0, 10.0):
        got = rf.ratio_from(M, sc["l2"], r, 0.8)
        assert got["idx"][1, 0] == 6 and np.isnan(got["dist"][1, 0]) and not got["keep"][1]
        assert got["keep"][0] and got["keep"][2] and tuple(got["idx"][[0, 2], 0]) == (2, 11)


def test_scene_g_one_column():
    sc, M = _special("single")
    for r in (-1.0, 0.0, 10.0):
        got = rf.ratio_from(M, sc["l2"], r, 0.8, mutual=True)
        assert (got["idx"] == [[0, -1]] * 5).all() and got["keep"].sum() == 1, "every row is kept by the ratio, one by the mutual check"
        assert rf.ratio_from(M, sc["l2"], r, 0.8)["count"] == 5


def test_scene_h_a_nan_centre_is_inconsistent_with_everything():
    sc, M = _special("nan_centre")
    assert tuple(gf.first_k(M[1:], np.ones((1, 12), bool), 3)[1][0]) == (8, 6, 5)
    got = rf.ratio_from(M, sc["l2"], 10.0, 0.8)
    plain = rf.ratio_from(M, sc["l2"], -1.0, 0.8)
    assert got["idx"][0, 0] == 4 and got["idx"][0, 1] == plain["idx"][0, 1] >= 0
    assert tuple(got["idx"][1]) == (8, 6)
    inc = rf.inconsistent(sc["l2"], np.array([8]), 10.0)[0]
    assert inc[5] and inc[6] and inc.sum() == 3 and inc[4]


def test_empty_sides():
    e = np.zeros((0, 128), F32)
    d = mf.planted(17, 33)[0]
    got = rf.ratio_from(mf.distance(d, e), rf.frames(np.zeros((0, 2))), 10.0, 0.8, mutual=True)
    assert got["count"] == 0 and (got["idx"] == -1).all() and np.isinf(got["dist"]).all() and got["dist"].shape == (17, 2)
    assert rf.ratio_from(mf.distance(e, d), rf.frames(np.zeros((17, 2))), 10.0, 0.8)["count"] == 0


# ---- the host side of the boundary ------------------------------------------------------------------------------------------------------
NEW = (("affnet_match_ratio_scratch_bytes", 3), ("affnet_match_ratio", 18), ("affnet_match_ratio_many_scratch_bytes", 4), ("affnet_match_ratio_many", 22))


def test_header_declares_and_lib_binds_the_entry_points():
    from affnet_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "affnet_hip.h")).read(), flags=re.S)
    for name, nargs in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(_lib.lib, name)
    assert re.search(r"#define\s+AFFNET_RATIO_MUTUAL\s+1\b", hdr) and _lib.RATIO_MUTUAL == 1


def test_python_api_has_the_matcher_keywords():
    import affnet_amd
    from affnet_amd import ReprojectionStuff as RS
    for name in ("enqueue_match_ratio", "match_ratio", "match_fginn"):
        assert getattr(affnet_amd, name) is getattr(RS, name)
    assert inspect.signature(RS.match_fginn).parameters["radius"].default == 10.0
    assert inspect.signature(RS.match_ratio).parameters["radius"].default is None
    fns = [RS.match_and_verify, RS.enqueue_match_and_verify_many, RS.match_and_verify_many, RS.spatial_rerank, affnet_amd.DescriptorIndex.retrieve]
    for f in fns:
        p = inspect.signature(f).parameters
        assert (p["matcher"].default, p["fginn_radius"].default, p["mutual"].default) == ("reference", 10.0, False), f
    for kw in (dict(matcher="sift"), dict(matcher="fginn", fginn_radius=-1.0), dict(matcher="fginn", fginn_radius=float("nan")), dict(mutual=True)):
        with pytest.raises(ValueError):
            RS.match_and_verify_many([], [], [], **kw)
        with pytest.raises(ValueError):
            RS.spatial_rerank([], [], 0, [], **kw)
    with pytest.raises(ValueError):
        RS.spatial_rerank([], [], 0, [], guided=True, matcher="fginn")
    for m in ("snn", "fginn"):
        assert RS.match_and_verify_many([], [], [], matcher=m, mutual=True) == []
        assert RS.spatial_rerank([], [], 0, [], matcher=m) == ([], [])


def test_scratch_bytes():
    from affnet_amd import _lib
    f, one = _lib.lib.affnet_match_ratio_many_scratch_bytes, _lib.lib.affnet_match_ratio_scratch_bytes
    Ps, ns, cs = (0, 1, 2, 3, 32, 1000, 65535), (0, 1, 15, 16, 17, 63, 64, 65, 200, 2000), (0, 1, 2, 3, 7, 64)
    mono = lambda v: all(y >= x for x, y in zip(v, v[1:]))
    for a in ns:
        for b in ns:
            for c in cs:
                assert mono([f(P, a, b, c) for P in Ps]), (a, b, c)
                for P in Ps:
                    assert f(P, a, b, c) >= P * (one(a, b, c) - 64), (P, a, b, c)
            # explicit chunk counts: more chunks, more partial lists; 0 = "the library chooses" is sized for the most it may choose
            assert mono([one(a, b, c) for c in range(1, 66)]) and one(a, b, 0) >= one(a, b, 1), (a, b)
            assert mono([f(3, a, b, c) for c in range(1, 66)]) and f(3, a, b, 0) >= f(3, a, b, 1), (a, b)
            # what the launches index: five arrays per row, three per column, the partial lists of both directions
            for c in cs[1:]:
                assert one(a, b, c) >= 4 * (5 * a + 3 * b) + 8 * max(2 * a * c, b * c), (a, b, c)
            assert one(a, b, 0) >= 4 * (5 * a + 3 * b) + 8 * max(2 * a * min(1024, max(1, (b + 15) // 16 // 5)), b * min(1024, max(1, (a + 15) // 16 // 5)))
    for c in cs:
        for b in ns:
            assert mono([one(a, b, c) for a in ns]) and mono([f(5, a, b, c) for a in ns]), (b, c)
        for a in ns:
            assert mono([one(a, b, c) for b in ns]) and mono([f(5, a, b, c) for b in ns]), (a, c)
    assert one(1, 1, 1) > 0 and f(1, 1, 1, 1) > 0
    assert one(-1, 50, 2) == one(0, 50, 2) and one(50, -1, 2) == one(50, 0, 2) and one(50, 50, -1) <= one(50, 50, 1)
    assert f(0, 0, 0, 0) == f(-3, 100, 100, 2) == f(0, 100, 100, 2)
    assert f(4, -1, 50, 2) == f(4, 0, 50, 2) and f(4, 50, -1, 2) == f(4, 50, 0, 2) and f(4, 50, 50, -1) <= f(4, 50, 50, 1)


def test_bad_arguments_are_refused_before_any_device_work():
    """The argument checks run on the host, in front of the first launch: they need no GPU."""
    from affnet_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == _lib.OK
    try:
        p = C.c_void_p(4096)            # never dereferenced: every call below is refused, or has no pair
        nan, inf = float("nan"), float("inf")
        ok = dict(d1=p, n1=20, d2=p, n2=20, dim=128, l2=p, r=10.0, thr=0.8, md=inf, flags=_lib.RATIO_MUTUAL, nc=0, dist=p, idx=p, tent=p, count=p, scr=p)

        def single(**kw):
            a = dict(ok, **kw)
            return lib.affnet_match_ratio(h, a["d1"], a["n1"], a["d2"], a["n2"], a["dim"], a["l2"], a["r"], a["thr"], a["md"], a["flags"], a["nc"], a["dist"],
                                          a["idx"], a["tent"], a["count"], a["scr"], None)
        bad = [dict(d1=None), dict(d2=None), dict(l2=None), dict(l2=None, r=0.0), dict(dist=None), dict(idx=None), dict(tent=None), dict(count=None), dict(scr=None),
               dict(n1=-1), dict(n2=-1), dict(dim=64), dict(flags=2), dict(flags=-1), dict(r=nan), dict(r=inf), dict(md=nan), dict(nc=-1), dict(nc=65536),
               dict(scr=C.c_void_p(4100)), dict(l2=None, r=-1.0, dim=64)]
        for kw in bad:
            assert single(**kw) == _lib.ERR_INVALID, kw
            assert b"match_ratio" in lib.affnet_last_error(h), kw
        assert lib.affnet_match_ratio(None, p, 20, p, 20, 128, p, 10.0, 0.8, inf, 1, 0, p, p, p, p, p, None) == _lib.ERR_INVALID

        mk = dict(ok, rows1=40, rows2=40, pairs=p, P=2)

        def many(**kw):
            a = dict(mk, **kw)
            return lib.affnet_match_ratio_many(h, a["d1"], a["rows1"], a["d2"], a["rows2"], a["dim"], a["l2"], a["pairs"], a["P"], a["n1"], a["n2"], a["r"],
                                               a["thr"], a["md"], a["flags"], a["nc"], a["dist"], a["idx"], a["tent"], a["count"], a["scr"], None)
        for kw in bad + [dict(pairs=None), dict(rows1=-1), dict(rows2=-1), dict(P=-1), dict(P=65536)]:
            assert many(**kw) == _lib.ERR_INVALID, kw
            assert b"match_ratio_many" in lib.affnet_last_error(h), kw
        assert many(P=0) == _lib.OK
        assert many(P=0, l2=None, r=-1.0, flags=0, nc=3) == _lib.OK and many(P=0, l2=None, r=-inf) == _lib.OK
        assert lib.affnet_match_ratio_many(None, p, 40, p, 40, 128, p, p, 2, 20, 20, 10.0, 0.8, inf, 1, 0, p, p, p, p, p, None) == _lib.ERR_INVALID
    finally:
        lib.affnet_ctx_destroy(h)
