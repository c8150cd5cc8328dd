"""CPU only: every planted construction of tests/_planted_onepass.py does, on the restatement of OnePassSIR alone, what it is named
after (so that tests/test_gpu_planted_onepass.py cannot pass vacuously), and _planted_onepass.select_rows_onepass - the rule the kernels
are held to - IS the oracle's own answer: for every case and budget the unmodified OnePassOracle(num_features=N) returns the same set
of (key, response bits), up to the members of a group of tied responses at a cut, where torch.topk leaves the choice open.

_planted_onepass.ALL_RUNS is the one list of (case, budget) pairs: the GPU file runs exactly these, and every check below walks all of
them."""
import numpy as np
import pytest
import torch

import _planted as pl
import _planted_onepass as po
import affnet_oracle as orc

rows_of, radix_budget, ALL_RUNS, RUN_IDS = po.rows_of, po.radix_budget, po.ALL_RUNS, po.RUN_IDS
# the ONLY runs compared in the weaker form (sets equal outside the tied group): the cut of the radix level falls inside a group of ties
TIE_RUNS = {("radix %s" % k, N) for k, N in po.RADIX_TIES}


def keyset(ids, resp):
    return set(zip(pl.order_key(np.asarray(ids).astype(np.int64)).tolist(), np.ascontiguousarray(resp, dtype=np.float32).view(np.uint32).tolist()))


def corners(norm):
    """(n, 2, 4) corners of the x 3.0 frames (OnePassSIR.py:95) of normalised LAFs, fp64"""
    L = torch.from_numpy(np.asarray(norm)).double()
    return orc.frame_corners(torch.cat([L[:, :2, :2] * 3.0, L[:, :, 2:]], dim=2)).numpy()


def test_the_run_list_is_complete():
    """nobody may quietly drop cases: the list holds every builder, every level / nlevels / budget of the switch and every radix run"""
    labels = [r[0] for r in ALL_RUNS]
    assert len(ALL_RUNS) == 2 + 1 + 18 + 2 + 1 + len(po.RADIX_RUNS) + 3 and len(set(RUN_IDS)) == len(RUN_IDS)
    for name in ("offdiag", "boundary", "cut_counts_positives below", "cut_counts_positives above", "cut_before_filter", "batch3 image 1"):
        assert name in labels
    assert {k for k, _, _ in po.RADIX_RUNS} == {"first", "last", "bucket0", "all equal"}
    assert TIE_RUNS <= {(r[0], r[2]) for r in ALL_RUNS} and po.RADIX_EXACT_TIES <= {(k, N) for k, _, N in po.RADIX_RUNS}
    for _, p, _, _ in ALL_RUNS:                      # the configuration the issue fixes: small images, every octave >= 34 px, |a_ij| <= 2
        shapes, _ = po.plan_of(p.case.H, p.case.W, p.case.kw.get("nlevels", 3))
        assert p.case.H <= 96 and p.case.W <= 160 and min(min(s) for s in shapes) >= 34 and len(p.maps) == len(shapes)
        assert max(float(m.abs().max()) for m in p.maps) <= 2.0


@pytest.mark.parametrize("run", ALL_RUNS, ids=RUN_IDS)
def test_the_rule_is_the_oracles(run):
    """select_rows_onepass(level_rows, N) against the unmodified OnePassOracle(num_features = N): the same set of (key, response bits);
    in the tie runs (TIE_RUNS, nothing else) the two may differ inside the tied group only."""
    label, p, N, value = run
    rows = rows_of(p, value)
    want = po.select_rows_onepass(rows, N)
    ex, L, r = po.run_oracle(p, N, value)
    got, exp = keyset(ex.keys.numpy(), r.numpy()), keyset(want["ids"], want["resp"])
    cuts = po.cut_report(rows, N)
    tied = [c for c in cuts.values() if c["ties"] > c["need"]]
    if (label, N) not in TIE_RUNS:
        assert not tied, "%s: an unnamed tie at a cut: %s" % (label, cuts)
        assert got == exp, "%s N=%d: %d rows differ" % (label, N, len(got ^ exp))
        # and the frames: the rows' pixel LAFs are the oracle's own, bit for bit
        pos = {k: i for i, k in enumerate(pl.order_key(want["ids"]).tolist())}
        idx = [pos[k] for k in pl.order_key(ex.keys.numpy().astype(np.int64)).tolist()]
        assert np.array_equal(want["lafs"][idx], L.numpy())
    else:
        assert len(tied) == 1 and len(got) == len(exp)
        tbits = int(np.float32(tied[0]["T"]).view(np.uint32))
        assert {b for _, b in got ^ exp} <= {tbits}, "%s: the sets differ outside the tied group" % label


@pytest.mark.parametrize("run", ALL_RUNS, ids=RUN_IDS)
def test_no_frame_sits_on_the_boundary(run):
    """every corner of every planted x 3.0 frame is at least 1e-4 normalised units from 0 and from 1 (fp32 rounding of centre and scale is
    three orders of magnitude below): the inside flag is decided by the construction, not by the last bit - read off the oracle's LAFs"""
    rows = rows_of(run[1], run[3])
    c = corners(rows["norm"])
    margin = np.minimum(np.abs(c), np.abs(1.0 - c)).min()
    assert margin >= 1e-4, margin
    outside = ((c < 0.0) | (c > 1.0)).any(axis=(1, 2))
    assert np.array_equal(outside, ~rows["inside"])


def test_offdiag_reaches_all_four_planes_in_both_octaves():
    p = po.offdiag()
    rows = rows_of(p)
    assert len(rows["resp"]) == 12 and rows["inside"].all() and sorted(set(map(tuple, rows["ids"][:, :2].tolist()))) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    seen = set()
    for (o, l, pix), n in zip(rows["ids"].tolist(), rows["norm"]):
        a = p.maps[o][0].reshape(4, -1)[:, pix].numpy()
        assert len(set(np.abs(a).tolist())) == 4 and np.all(np.abs(a) >= 0.25)                   # four non-zero, distinct entries
        s = np.float64(n[0, 0]) / np.float64(a[0])
        assert np.allclose(n[:, :2].reshape(4), s * a.astype(np.float64), rtol=1e-6)             # the frame is s A of THIS pixel, plane by plane
        seen.add(tuple(a.tolist()))
    assert len(seen) == 12                                                                       # and no two maxima share a map
    assert not np.array_equal(po.select_rows_onepass(rows, 4)["ids"], rows["ids"][:4])           # N = 4: response order crosses the octaves
    assert len(set(po.select_rows_onepass(rows, 4)["ids"][:, 0].tolist())) == 2


def test_boundary_rows_fail_exactly_the_named_inequality():
    p = po.boundary()
    rows = rows_of(p)
    assert len(rows["resp"]) == 12 and int(rows["inside"].sum()) == 6
    c = corners(rows["norm"])
    W = p.case.W
    for name, ((yo, xo), (yi, xi)) in po.BOUNDARY_SPOTS.items():
        io, ii = [int(np.nonzero(rows["ids"][:, 2] == y * W + x)[0][0]) for y, x in ((yo, xo), (yi, xi))]
        ox, oy = c[io, 0], c[io, 1]
        fails = {"ox<0": int((ox < 0).sum()), "ox>1": int((ox > 1).sum()), "oy<0": int((oy < 0).sum()), "oy>1": int((oy > 1).sum())}
        want = {k: int(k == po.BOUNDARY_EDGES[name]) for k in fails}
        assert fails == want, (name, fails)                                    # exactly one corner, through exactly this inequality
        assert not rows["inside"][io] and rows["inside"][ii], name             # and the twin stays
        if name.endswith("only"):                                              # the diagonal terms alone would keep the frame inside
            n = rows["norm"][io:io + 1].copy()
            n[0, 0, 1] = 0.0
            n[0, 1, 0] = 0.0
            cd = corners(n)
            assert ((cd >= 1e-4) & (cd <= 1.0 - 1e-4)).all(), name
            off = p.maps[0][0, 1 if name == "a12 only" else 2, yo, xo]
            other = p.maps[0][0, 2 if name == "a12 only" else 1, yo, xo]
            assert abs(float(off)) > 2.0 * abs(float(other))                   # the two off-diagonal planes are not interchangeable here
    assert set(failed_inequalities(rows, c)) == {"ox<0", "ox>1", "oy<0", "oy>1"}


def failed_inequalities(rows, c):
    out = []
    for i in np.nonzero(~rows["inside"])[0]:
        out += [k for k, m in (("ox<0", c[i, 0] < 0), ("ox>1", c[i, 0] > 1), ("oy<0", c[i, 1] < 0), ("oy>1", c[i, 1] > 1)) if m.any()]
    return out


@pytest.mark.parametrize("nlevels", [3, 4])
@pytest.mark.parametrize("level", [1, 2, "last"])
def test_cut_switch_sits_on_the_switch(level, nlevels):
    p = po.cut_switch(level, nlevels)
    rows = rows_of(p)
    l1 = (nlevels if level == "last" else level) - 1
    at = rows["ids"][:, 1] == l1
    r = rows["resp"][at]
    assert int((r > 0).sum()) == po.CUT_P and int((~rows["inside"][at]).sum()) == po.CUT_OUT
    assert set(np.sort(r)[::-1][:po.CUT_OUT].tolist()) == set(r[~rows["inside"][at]].tolist())       # the largest are the ones outside
    assert int((r < 0).sum()) == (0 if l1 == 0 else 1)                                              # level 1 has no octaveMap below it
    others = [int((rows["ids"][:, 1] == l).sum()) for l in range(nlevels) if l != l1]
    assert min(others) >= 2 and sum(others) < po.CUT_OUT                 # every level is applied; the global budget never fires
    assert list(po.cut_report(rows, po.CUT_P - 1)) == [(0, l1)] and not po.cut_report(rows, po.CUT_P) and not po.cut_report(rows, po.CUT_P + 1)
    n = {d: po.select_rows_onepass(rows, po.CUT_P + d) for d in (-1, 0, 1)}
    in_level = {d: n[d]["ids"][:, 1] == l1 for d in n}
    assert int(in_level[-1].sum()) == po.CUT_P - 1 - po.CUT_OUT          # cut: the 40th positive and the negative row go, nothing is promoted
    assert int(in_level[0].sum()) == int(in_level[1].sum()) == po.CUT_P - po.CUT_OUT + (1 if l1 else 0)
    if l1:
        assert (n[0]["resp"][in_level[0]] < 0).sum() == 1 and (n[-1]["resp"] > 0).all()


def test_cut_counts_positives_not_raw_maxima():
    for variant, n_pos, neg in (("below", po.COUNTS_N - 1, 2), ("above", po.COUNTS_N + 1, 1)):
        rows = rows_of(po.cut_counts_positives(variant))
        at = rows["ids"][:, 1] == 2
        r = rows["resp"][at]
        assert len(r) + (1 if variant == "below" else 0) == po.COUNTS_N + 2            # raw maxima: one of "below" became a zero, no row
        assert int((r > 0).sum()) == n_pos and int((r < 0).sum()) == neg
        cut = po.cut_report(rows, po.COUNTS_N)
        want = po.select_rows_onepass(rows, po.COUNTS_N)
        assert len(want["resp"]) < po.COUNTS_N                                         # the global budget does not hide what the level did
        if variant == "below":
            assert not cut and int((want["resp"] < 0).sum()) == 2
        else:
            assert list(cut) == [(0, 2)] and (want["resp"] > 0).all()
            assert int((want["ids"][:, 1] == 2).sum()) == po.COUNTS_N - 10


def test_cut_before_filter_promotes_nothing():
    p = po.cut_before_filter()
    rows = rows_of(p)
    N = po.BEFORE_N
    at = (rows["ids"][:, 0] == 0) & (rows["ids"][:, 1] == 1)
    r = rows["resp"][at]
    assert len(r) == N + 6 and (r > 0).all()
    assert set(np.sort(r)[::-1][:5].tolist()) == set(r[~rows["inside"][at]].tolist()) and int((~rows["inside"]).sum()) == 5
    assert list(po.cut_report(rows, N)) == [(0, 1)]
    want = po.select_rows_onepass(rows, N)
    lvl = (want["ids"][:, 0] == 0) & (want["ids"][:, 1] == 1)
    assert int(lvl.sum()) == N - 5 and len(want["resp"]) == N                  # N - 5 of the level + the five rows of the uncut levels
    assert float(want["resp"][lvl].min()) == float(np.sort(r)[::-1][N - 1])   # rank N is the last one kept, ranks N + 1 .. N + 6 are gone
    rest = want["resp"][~lvl]
    assert len(rest) == 5 and float(rest.max()) < float(want["resp"][lvl].min())      # under the cut level's threshold they would vanish
    assert sorted(set(map(tuple, want["ids"][~lvl][:, :2].tolist()))) == [(0, 2), (1, 1)]


def radix_key(resp):
    """detect.hip order_key(): larger float -> larger uint32"""
    u = np.ascontiguousarray(resp, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


@pytest.mark.parametrize("kind,n_out,N", po.RADIX_RUNS, ids=["%s-out%d-N%s" % r for r in po.RADIX_RUNS])
def test_radix_cases_decide_where_they_say(kind, n_out, N):
    """replays the MSB-first 8-bit select of onepass_level_select_kernel on the oracle's rows of the radix level"""
    edge = N is None
    N = radix_budget(kind, n_out, N)
    rows = rows_of(po.radix(kind, n_out))
    at = rows["ids"][:, 1] == 2
    r = rows["resp"][at]
    k = radix_key(r)
    assert int((r < 0).sum()) == 2 and int((r > 0).sum()) > N and int((~rows["inside"][at]).sum()) == n_out
    assert (k[r < 0] < 0x80000000).all() and (k[r > 0] >= 0x80000000).all()      # the negative rows sit in the histogram, below every positive
    need, prefix, mask, trace = N, 0, 0, []
    for shift in (24, 16, 8, 0):
        sel = k[(k & mask) == prefix]
        hist = np.bincount(((sel >> shift) & 255).astype(np.int64), minlength=256)
        d = 255
        while d > 0 and hist[d] < need:
            need -= int(hist[d])
            d -= 1
        trace.append({"buckets": int((hist > 0).sum()), "d": d, "need": need, "in_bucket": int(hist[d]), "fell_through": d == 0})
        prefix |= d << shift
        mask |= 255 << shift
    ties = int((k == prefix).sum())
    print(kind, N, trace, "ties", ties)
    rep = po.cut_report(rows, N)[(0, 2)]
    assert (rep["ties"], rep["need"]) == (ties, need)
    assert ((kind, N) in po.RADIX_TIES) == (ties > need) and ((kind, N) in po.RADIX_EXACT_TIES) == (ties == need and ties > 1)
    if kind == "first":
        assert trace[0]["buckets"] >= 10 + 1                                        # many first bytes (+ the negative rows')
        if edge:
            assert trace[0]["need"] == trace[0]["in_bucket"] > 1                    # the first byte decides alone: its bucket is taken whole
        elif N > 1:
            assert 1 <= trace[0]["need"] < trace[0]["in_bucket"]
        else:
            assert trace[0]["need"] == 1 and n_out == 0
    if kind == "last":
        pos = k[r > 0]
        assert len(np.unique(pos >> 8)) == 1 and len(np.unique(pos)) > 30           # three shared bytes, the last decides alone
        assert all(t["in_bucket"] == len(pos) for t in trace[:3]) and ties > need >= 1
    if kind == "bucket0":
        assert [t["fell_through"] for t in trace] == [False, True, True, True]      # bucket d == 0 of bytes 2, 1 and 0
        assert float(np.sort(r)[::-1][N - 1]) == 8.0 and ties == 6 and need == (3 if N == 31 else 6)
    if kind == "all equal":
        assert len(np.unique(r[r > 0])) == 1 and ties == 60 and need == N
        want = po.select_rows_onepass(rows, N)
        lvl = want["ids"][:, 1] == 2
        first = np.sort(rows["ids"][at][r > 0][:, 2])[:N]                           # pixel order decides ...
        assert set(want["ids"][lvl][:, 2].tolist()) == set(first.tolist()) - set(rows["ids"][at][~rows["inside"][at]][:, 2].tolist())
        assert int(lvl.sum()) == N - n_out                                          # ... and the filter's losses are not refilled


def test_batch_images_differ_where_it_matters():
    ps = po.batch3()
    rows = [rows_of(p, float(b)) for b, p in enumerate(ps)]
    N = po.BATCH_N
    assert list(po.cut_report(rows[0], N)) == [(0, 1)] and not po.cut_report(rows[1], N) and ps[2] == ps[0]
    assert not torch.equal(ps[0].maps[0], ps[1].maps[0])
    T = np.sort(rows[0]["resp"][rows[0]["ids"][:, 1] == 1])[::-1][N - 1]
    l1 = rows[1]["resp"][rows[1]["ids"][:, 1] == 1]
    assert (l1 < T).all() and int((l1 > 0).sum()) == 30                 # read through image 0's table, image 1's level would be emptied
    w0, w1 = po.select_rows_onepass(rows[0], N), po.select_rows_onepass(rows[1], N)
    assert len(w0["resp"]) != len(w1["resp"])
    # the slot callables find the image by its value whatever the level
    fn = po.by_image_value([lambda level, *a, b=b: b for b in range(3)])
    for b in range(3):
        assert fn(torch.full((1, 1, 40, 50), b * 1.00001), 1.6) == b


def test_planted_aff_fn_copies_and_finds_the_octave():
    p = po.offdiag()
    fn = po.planted_aff_fn(p.case.H, p.case.W, p.maps)
    for o in (1, 0, 1):
        got = fn(torch.zeros(1, 1, *p.maps[o].shape[2:]))
        assert torch.equal(got, p.maps[o])
        got[...] = 9.0
    assert float(p.maps[0].max()) <= 2.0


def test_select_rows_onepass_is_the_stated_rule():
    ids = np.array([[0, 0, 3], [0, 0, 5], [0, 0, 9], [0, 0, 11], [0, 1, 2], [0, 1, 4], [1, 0, 1]], dtype=np.int64)
    rows = {"ids": ids, "resp": np.array([5.0, 7.0, 5.0, -1.0, 2.0, 3.0, 6.0], dtype=np.float32), "lafs": np.zeros((7, 2, 3), np.float32),
            "inside": np.array([1, 0, 1, 1, 1, 1, 1], dtype=bool)}
    # N = 2 < n_pos = 3 of level (0, 0): 7.0 and the FIRST 5.0 in pixel order; 7.0 is outside and is not replaced by the other 5.0
    assert po.level_cut(rows, 2).tolist() == [True, True, False, False, True, True, True]
    assert po.select_rows_onepass(rows, 2)["ids"].tolist() == [[1, 0, 1], [0, 0, 3]]
    # N = 3 = n_pos: no cut, the negative row stays; five rows are left after the filter, the best three in response order
    assert po.level_cut(rows, 3).all()
    assert po.select_rows_onepass(rows, 3)["ids"].tolist() == [[1, 0, 1], [0, 0, 3], [0, 0, 9]]
    # N >= the rows left: (octave, level, pixel) order, negative row included
    assert po.select_rows_onepass(rows, 6)["ids"].tolist() == [[0, 0, 3], [0, 0, 9], [0, 0, 11], [0, 1, 2], [0, 1, 4], [1, 0, 1]]
    assert po.select_rows_onepass(rows, -1)["ids"].tolist() == po.select_rows_onepass(rows, 6)["ids"].tolist()
