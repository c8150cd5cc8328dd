"""MI355X: epipolar verification and guided matching of many image pairs in one device call (affnet_epipolar_verify_many,
affnet_match_guided_many; ReprojectionStuff.match_and_verify_many(model="fundamental"), match_verify_guided_many, spatial_rerank(guided=True),
DescriptorIndex.retrieve(guided=True)) against the single-pair calls, which tests/test_gpu_epipolar.py and tests/test_gpu_guided.py pin to their
restatements.  The batched kernels run the single-pair device functions on each pair's segments, so the tolerance is zero: every comparison
below is on the bytes."""
import numpy as np
import pytest
import torch

import _epipolar_fp64 as ep
import _guided_fp32 as gf
import _spatial_fp64 as sp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TH = 2.0
INF = float("inf")
SENT_F32, SENT_I32, SENT_U8 = -7.5, -7, 0xAB
# (T, outlier share, seed): one below, at and one above the solve tile (64) and the scoring tile and chunk (128), more than one of each; T < 3
# (no hypothesis) and fewer than 8 inliers (no refit)
EPI_SCENES = [(2, 0, 3), (3, 0, 4), (7, 0, 5), (8, 0, 6), (9, 0, 16), (63, .3, 7), (64, .3, 8), (65, .3, 9), (127, .5, 10), (128, .5, 11), (129, .5, 12),
              (257, .5, 13)]
DENSE = [(1, 1), (15, 17), (16, 16), (23, 40), (63, 80), (64, 79), (65, 81), (130, 200)]
COUNTS = [1, 15, 16, 17, 63, 64, 65, 130, 200]       # the ragged image set of the table guard (tests/test_gpu_match_many.py)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _api():
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device(DEV)
    return lib, ptr, check, engine.utility_ctx(dev), engine.stream_of(dev), dev


def full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def dev_of(x, dtype=np.float32):
    return torch.from_numpy(np.array(x, dtype)).to(DEV)          # a copy: the scenes are read-only


# ---- the raw calls, on buffers pre-filled with sentinels so that "not written" can be seen ---------------------------------------------------
def raw_epi(l1, l2, tent, rounds, lo_iters, seed=0, count=None, th=TH):
    """affnet_epipolar_verify on device frames and a (cap,2) numpy tentative list; count: the device-side row count, or None = all rows."""
    lib, ptr, check, ctx, st, dev = _api()
    cap = tent.shape[0]
    dt = torch.zeros(max(cap, 1), 2, dtype=torch.int32, device=dev)
    dt[:cap] = torch.from_numpy(np.ascontiguousarray(tent, np.int32)).to(dev)
    dc = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    counts, inl = full((max(cap * rounds, 1),), SENT_I32, torch.int32), full((max(cap, 1),), SENT_U8, torch.uint8)
    F, summ = full((9,), float("nan"), torch.float64), full((4,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_epipolar_scratch_bytes(cap, rounds), dtype=torch.uint8, device=dev)
    check(lib.affnet_epipolar_verify(ctx, ptr(l1), l1.size(0), ptr(l2), l2.size(0), ptr(dt), ptr(dc), cap, th, rounds, seed, lo_iters, ptr(counts), ptr(F), ptr(inl),
                                     ptr(summ), ptr(scratch), st), ctx, "affnet_epipolar_verify")
    return dict(counts=counts.cpu().numpy()[:cap * rounds], inlier=inl.cpu().numpy()[:cap], F=F.cpu().numpy(), summary=summ.cpu().numpy())


def raw_epi_many(L1, L2, table, d_tent, d_count, t_max, rounds, lo_iters, seed=0, th=TH):
    lib, ptr, check, ctx, st, dev = _api()
    P = table.shape[0]
    counts, inl = full((P, max(t_max * rounds, 1)), SENT_I32, torch.int32), full((P, max(t_max, 1)), SENT_U8, torch.uint8)
    F, summ = full((P, 9), float("nan"), torch.float64), full((P, 4), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_epipolar_many_scratch_bytes(P, t_max, rounds), dtype=torch.uint8, device=dev)
    pairs = torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev)
    check(lib.affnet_epipolar_verify_many(ctx, ptr(L1), L1.size(0), ptr(L2), L2.size(0), ptr(pairs), P, ptr(d_tent), ptr(d_count), t_max, th, rounds, seed, lo_iters,
                                          ptr(counts), ptr(F), ptr(inl), ptr(summ), ptr(scratch), st), ctx, "affnet_epipolar_verify_many")
    return dict(counts=counts.cpu().numpy(), inlier=inl.cpu().numpy(), F=F.cpu().numpy(), summary=summ.cpu().numpy())


def raw_guided(d1, d2, l1, l2, model, kind, r, thr, mutual, gate=None, n_chunks=0):
    """affnet_match_guided on device tensors (model (9,) float64, gate (4,) int32 or None) -> numpy dict."""
    lib, ptr, check, ctx, st, dev = _api()
    n1, n2 = d1.size(0), d2.size(0)
    dist, idx = full((max(n1, 1), 2), SENT_F32, torch.float32), full((max(n1, 1), 2), SENT_I32, torch.int32)
    tent, cnt = full((max(n1, 1), 2), SENT_I32, torch.int32), full((1,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_match_guided_scratch_bytes(n1, n2, n_chunks), dtype=torch.uint8, device=dev)
    check(lib.affnet_match_guided(ctx, ptr(d1), n1, ptr(d2), n2, 128, ptr(l1), ptr(l2), ptr(model), kind, r, thr, INF, 1 if mutual else 0, n_chunks, ptr(gate),
                                  ptr(dist), ptr(idx), ptr(tent), ptr(cnt), ptr(scratch), st), ctx, "affnet_match_guided")
    return dict(dist=dist.cpu().numpy()[:n1], idx=idx.cpu().numpy()[:n1], tent=tent.cpu().numpy()[:n1], count=int(cnt.item()))


def raw_guided_many(D1, D2, L1, L2, table, n1_max, n2_max, models, kind, r, thr, mutual, gates=None, n_chunks=0):
    lib, ptr, check, ctx, st, dev = _api()
    P = table.shape[0]
    dist, idx = full((P, max(n1_max, 1), 2), SENT_F32, torch.float32), full((P, max(n1_max, 1), 2), SENT_I32, torch.int32)
    tent, cnt = full((P, max(n1_max, 1), 2), SENT_I32, torch.int32), full((P,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_match_guided_many_scratch_bytes(P, n1_max, n2_max, n_chunks), dtype=torch.uint8, device=dev)
    pairs = torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev)
    check(lib.affnet_match_guided_many(ctx, ptr(D1), D1.size(0), ptr(D2), D2.size(0), 128, ptr(L1), ptr(L2), ptr(pairs), P, n1_max, n2_max, ptr(models), kind, r, thr,
                                       INF, 1 if mutual else 0, n_chunks, ptr(gates), ptr(dist), ptr(idx), ptr(tent), ptr(cnt), ptr(scratch), st), ctx,
          "affnet_match_guided_many")
    return dict(dist=dist.cpu().numpy(), idx=idx.cpu().numpy(), tent=tent.cpu().numpy(), count=cnt.cpu().numpy())


def check_guided_pair(got, p, want, n1, what):
    k = want["count"]
    assert got["count"][p] == k, (what, int(got["count"][p]), k)
    assert same(got["dist"][p, :n1], want["dist"]) and same(got["idx"][p, :n1], want["idx"]), what
    assert same(got["tent"][p, :k], want["tent"][:k]), what
    assert (got["tent"][p, k:] == SENT_I32).all() and (want["tent"][k:] == SENT_I32).all(), (what, "tent rows at or beyond the count are not written")
    assert (got["dist"][p, n1:] == SENT_F32).all() and (got["idx"][p, n1:] == SENT_I32).all(), (what, "rows n1 .. n1_max are not written")


# ---- inputs, computed once and never modified ----------------------------------------------------------------------------------------------------
_CACHE = {}


def epi_set():
    """The 12 planted scenes with depth back to back, their pair table and the pair-major tentative lists."""
    if "epi" not in _CACHE:
        cases = [ep.planted_two_view(T, share, seed) for T, share, seed in EPI_SCENES]
        Ts = [T for T, _, _ in EPI_SCENES]
        t_max = max(Ts)
        off = np.concatenate([[0], np.cumsum(Ts)])
        table = np.array([[off[p], Ts[p], off[p], Ts[p]] for p in range(len(Ts))], np.int32)
        tent = np.full((len(Ts), t_max, 2), 1 << 20, np.int32)          # rows behind a pair's count: an index far outside, never read
        for p, c in enumerate(cases):
            tent[p, :Ts[p]] = c[2]
        _CACHE["epi"] = dict(cases=cases, Ts=Ts, t_max=t_max, table=table, L1=dev_of(np.concatenate([c[0] for c in cases])),
                             L2=dev_of(np.concatenate([c[1] for c in cases])), d_tent=torch.from_numpy(tent).to(DEV),
                             d_count=torch.tensor(Ts, dtype=torch.int32, device=DEV),
                             l1=[dev_of(c[0]) for c in cases], l2=[dev_of(c[1]) for c in cases])
    return _CACHE["epi"]


def guided_set():
    """The guided scenes back to back: the eight dense scenes, then the repeated scene of either kind."""
    if "guided" not in _CACHE:
        scenes = [gf.dense_scene(n1, n2) for n1, n2 in DENSE] + [gf.repeated_scene(257, 257, gf.PLANAR), gf.repeated_scene(257, 258, gf.EPIPOLAR)]
        c1, c2 = [s["d1"].shape[0] for s in scenes], [s["d2"].shape[0] for s in scenes]
        o1, o2 = np.concatenate([[0], np.cumsum(c1)]), np.concatenate([[0], np.cumsum(c2)])
        table = np.array([[o1[p], c1[p], o2[p], c2[p]] for p in range(len(scenes))], np.int32)
        cat = lambda k: dev_of(np.concatenate([s[k] for s in scenes]))
        _CACHE["guided"] = dict(scenes=scenes, table=table, n1_max=max(c1), n2_max=max(c2), D1=cat("d1"), D2=cat("d2"), L1=cat("l1"), L2=cat("l2"),
                                each=[{k: dev_of(s[k]) for k in ("d1", "d2", "l1", "l2")} for s in scenes])
    return _CACHE["guided"]


def guided_models(kind):
    """One model row per pair, every row different: the scene's own model where it is of this kind, the dense scenes' model of this kind
    elsewhere, each moved by a pair-dependent amount."""
    g = guided_set()
    rows = []
    for p, s in enumerate(g["scenes"]):
        own = p == len(DENSE) + (0 if kind == gf.PLANAR else 1)
        if kind == gf.PLANAR:
            m = np.array(s["model"] if own else gf.DENSE_H, np.float64).reshape(3, 3)
            m[0, 2] += 0.75 * p
            m[1, 2] -= 0.5 * p
        else:
            m = np.array(s["model"] if own else ep.planted_F(), np.float64).reshape(3, 3) * (1.0 + p / 16.0)
            m[2, 2] += 1e-3 * p
        rows.append(m.reshape(9))
    return torch.from_numpy(np.stack(rows)).to(DEV)


def image_set():
    """tests/test_gpu_match_many.py's ragged image set: unit descriptors that are noisy copies of rows of one pool, random frames."""
    if "images" not in _CACHE:
        rng = np.random.default_rng(11)
        pool = rng.normal(size=(200, 128))
        descs, lafs = [], []
        for n in COUNTS:
            d = pool[rng.permutation(200)[:n]] + 0.06 * rng.normal(size=(n, 128))
            descs.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
            lafs.append(sp.random_frames(rng, n).astype(np.float32))
        _CACHE["images"] = dict(off=np.concatenate([[0], np.cumsum(COUNTS)]), D=dev_of(np.concatenate(descs)), L=dev_of(np.concatenate(lafs)))
    return _CACHE["images"]


def _recorded_calls():
    """One affnet_epipolar_verify and one affnet_match_guided call -> their outputs."""
    e, g = epi_set(), guided_set()
    p = EPI_SCENES.index((129, .5, 12))
    v = raw_epi(e["l1"][p], e["l2"][p], e["cases"][p][2], 8, 3)
    q = DENSE.index((130, 200))
    s = g["each"][q]
    m = raw_guided(s["d1"], s["d2"], s["l1"], s["l2"], dev_of(gf.DENSE_H.reshape(9), np.float64), gf.PLANAR, gf.DENSE_R, 0.9, True)
    return v, m


@pytest.fixture(scope="module", autouse=True)
def recorded_single_pair_calls():
    """Outputs of the single-pair entry points, recorded before the first batched call of this module (this fixture runs in front of its first test)."""
    return _recorded_calls()


# ---- 1. epipolar verification: many equals the loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo_iters", [3, 0])
@pytest.mark.parametrize("rounds", [1, 3, 8])
def test_epipolar_verification_equals_the_loop(rounds, lo_iters):
    """Condition on the inputs: the float64 restatement tests/_epipolar_fp64.verify (th = 2, seed 0, lo_iters = 3), run on the CPU, gives flag 1
    for T = 2, flag 2 for T = 3 .. 9 and flag 0 for all seven T >= 63, at each of rounds 1, 3 and 8.  Flag 2 is raised inside the refit loop, so
    with lo_iters = 0 no call can carry it: that run is asked for flag 1 and for six flag-free pairs only."""
    e = epi_set()
    got = raw_epi_many(e["L1"], e["L2"], e["table"], e["d_tent"], e["d_count"], e["t_max"], rounds, lo_iters)
    flags = []
    for p, c in enumerate(e["cases"]):
        T = e["Ts"][p]
        want = raw_epi(e["l1"][p], e["l2"][p], c[2], rounds, lo_iters)
        flags.append(int(want["summary"][3]))
        print("T = %d rounds = %d lo_iters = %d: summary %s" % (T, rounds, lo_iters, want["summary"].tolist()))
        assert same(got["summary"][p], want["summary"]) and same(got["F"][p], want["F"]), (T, got["summary"][p], want["summary"])
        assert same(got["counts"][p, :T * rounds], want["counts"]) and same(got["inlier"][p, :T], want["inlier"]), T
        assert (got["counts"][p, T * rounds:] == SENT_I32).all() and (got["inlier"][p, T:] == SENT_U8).all(), "rows at or beyond the count are not written"
    assert flags.count(0) >= 6 and 1 in flags, flags
    if lo_iters:
        assert 2 in flags, flags
    again = raw_epi_many(e["L1"], e["L2"], e["table"], e["d_tent"], e["d_count"], e["t_max"], rounds, lo_iters)
    assert all(same(again[k], got[k]) for k in got), "same bytes every run"


def test_epipolar_verification_without_a_count():
    """d_count = NULL: t_max rows are valid in every pair."""
    cases = [ep.planted_two_view(65, .3, 9), ep.planted_two_view(65, .3, 19)]
    L1, L2 = dev_of(np.concatenate([c[0] for c in cases])), dev_of(np.concatenate([c[1] for c in cases]))
    table = np.array([[0, 65, 0, 65], [65, 65, 65, 65]], np.int32)
    d_tent = torch.from_numpy(np.stack([c[2] for c in cases]).astype(np.int32)).to(DEV)
    got = raw_epi_many(L1, L2, table, d_tent, None, 65, 8, 3, seed=5)
    for p, c in enumerate(cases):
        want = raw_epi(dev_of(c[0]), dev_of(c[1]), c[2], 8, 3, seed=5)
        assert all(same(got[k][p], want[k]) for k in want), p
        assert want["summary"][3] == 0 and want["summary"][2] >= 8
    assert not same(got["F"][0], got["F"][1])


# ---- 2. guided matching: many equals the loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("kind", [gf.PLANAR, gf.EPIPOLAR])
def test_guided_matching_equals_the_loop(kind, mutual):
    g = guided_set()
    P = len(g["scenes"])
    models = guided_models(kind)
    r = gf.DENSE_R          # for either kind, as tests/test_gpu_guided.py uses the dense scenes: the float32 restatement keeps matches in every pair
    gate_rows = np.array([[-1, 0, 0, 1] if p % 3 == 1 else ([3, 9, 9, 2] if p % 3 == 2 else [5, 20, 31, 0]) for p in range(P)], np.int32)
    kept = {}
    for gates in (None, torch.from_numpy(gate_rows).to(DEV)):
        wants = []
        for p, s in enumerate(g["each"]):
            wants.append(raw_guided(s["d1"], s["d2"], s["l1"], s["l2"], models[p], kind, r, 0.9, mutual, None if gates is None else gates[p]))
        first = None
        for nc in (0, 1, 2, 3):
            got = raw_guided_many(g["D1"], g["D2"], g["L1"], g["L2"], g["table"], g["n1_max"], g["n2_max"], models, kind, r, 0.9, mutual, gates, nc)
            for p in range(P):
                check_guided_pair(got, p, wants[p], int(g["table"][p, 1]), (kind, mutual, gates is not None, nc, p))
            first = got if first is None else first
            assert all(same(got[k], first[k]) for k in got), ("the result does not depend on the chunks", nc)
        kept[gates is None] = [w["count"] for w in wants]
        if gates is not None:
            for p in range(P):
                if gate_rows[p, 3] & 1:
                    n1 = int(g["table"][p, 1])
                    assert first["count"][p] == 0 and (first["idx"][p, :n1] == -1).all() and np.isinf(first["dist"][p, :n1]).all(), "a closed gate: unfilled lists"
    print("kind %d mutual %s: kept per pair %s (no gate), %s (gates)" % (kind, mutual, kept[True], kept[False]))
    assert all(k > 0 for k in kept[True]), "the scenes have matches to keep"
    assert [k for p, k in enumerate(kept[False]) if p % 3 != 1] == [k for p, k in enumerate(kept[True]) if p % 3 != 1], "other flags leave the gate open"


# ---- 3. the pair table is tested before anything is loaded or stored through it ----------------------------------------------------------------------
def _guard_table():
    s = image_set()
    off, rows = s["off"], int(s["off"][-1])
    i3, i6, i7, i8 = int(off[3]), int(off[6]), int(off[7]), int(off[8])
    big = 0x7fffffff
    table = np.array([[i3, 17, i7, 130],            # 0 valid
                      [-1, 17, i7, 130],            # 1 negative row1
                      [i3, 17, i7, -130],           # 2 negative n2
                      [rows - 3, 17, i7, 130],      # 3 row1 + n1 > rows1
                      [i3, 17, rows - 3, 130],      # 4 row2 + n2 > rows2
                      [i7, 130, i3, 17],            # 5 n1 > n1_max
                      [i3, 17, i7, 0],              # 6 empty side 2
                      [i3, 0, i7, 130],             # 7 empty side 1
                      [big, big, i7, 130],          # 8 row1 + n1 beyond int32
                      [i6, 65, i3, 17],             # 9 valid, n1 at the cap
                      [i3, 17, i8, 200]], np.int32)  # 10 n2 > n2_max
    return table, 65, 130, [1, 2, 3, 4, 5, 8], [6, 7], [0, 9]


def test_table_guard_epipolar():
    lib, ptr, check, ctx, st, dev = _api()
    s = image_set()
    table, n1_max, n2_max, bad, empty, valid = _guard_table()
    P = table.shape[0]
    # the tentative lists of affnet_match_snn_many, as in the chain
    md, md2, idx = full((P, n1_max), SENT_F32, torch.float32), full((P, n1_max), SENT_F32, torch.float32), full((P, n1_max), SENT_I32, torch.int32)
    d_tent, d_count = full((P, n1_max, 2), SENT_I32, torch.int32), full((P,), SENT_I32, torch.int32)
    scratch = torch.empty(lib.affnet_match_many_scratch_bytes(P, n1_max, n2_max), dtype=torch.uint8, device=dev)
    pairs = torch.from_numpy(table).to(dev)
    check(lib.affnet_match_snn_many(ctx, ptr(s["D"]), s["D"].size(0), ptr(s["D"]), s["D"].size(0), 128, ptr(pairs), P, n1_max, n2_max, 0.8, ptr(md), ptr(idx),
                                    ptr(md2), ptr(d_tent), ptr(d_count), ptr(scratch), st), ctx, "affnet_match_snn_many")
    tent, count = d_tent.cpu().numpy(), d_count.cpu().numpy()
    rounds = 3
    v = raw_epi_many(s["L"], s["L"], table, d_tent, d_count, n1_max, rounds, 3, th=3.0)
    for p in bad + empty + [10]:
        assert count[p] == 0, p
        assert (v["counts"][p] == SENT_I32).all() and (v["inlier"][p] == SENT_U8).all(), p
        assert same(v["F"][p], np.zeros(9)), (p, "the zero model of flag 1, not the identity")
    for p in bad:
        assert v["summary"][p].tolist() == [-1, 0, 0, 9], (p, v["summary"][p])
    for p in empty + [10]:      # (the verification has no cap on n2: a row that only the matcher's n2_max refuses is an empty list to it)
        assert v["summary"][p].tolist() == [-1, 0, 0, 1], (p, v["summary"][p])
    for p in valid:
        r1, n1, r2, n2 = table[p].tolist()
        k = int(count[p])
        assert k > 0
        want = raw_epi(s["L"][r1:r1 + n1], s["L"][r2:r2 + n2], tent[p, :k], rounds, 3, th=3.0)
        assert same(v["counts"][p, :k * rounds], want["counts"]) and same(v["inlier"][p, :k], want["inlier"]), p
        assert same(v["summary"][p], want["summary"]) and same(v["F"][p], want["F"]), p
        assert (v["counts"][p, k * rounds:] == SENT_I32).all() and (v["inlier"][p, k:] == SENT_U8).all()


@pytest.mark.parametrize("n_chunks", [0, 2])
def test_table_guard_guided(n_chunks):
    s = image_set()
    table, n1_max, n2_max, bad, empty, valid = _guard_table()
    P = table.shape[0]
    # random frames spread over the image: a wide radius under the identity admits a part of the columns
    models = torch.from_numpy(np.tile(np.eye(3).reshape(1, 9), (P, 1))).to(DEV)
    r = 300.0
    got = raw_guided_many(s["D"], s["D"], s["L"], s["L"], table, n1_max, n2_max, models, gf.PLANAR, r, 0.9, True, None, n_chunks)
    for p in bad + [7, 10]:      # out of range (here n2 has a cap too), or no row in image 1: count 0, nothing else written
        assert got["count"][p] == 0, p
        assert (got["dist"][p] == SENT_F32).all() and (got["idx"][p] == SENT_I32).all() and (got["tent"][p] == SENT_I32).all(), p
    # no row in image 2: what affnet_match_guided does - count 0, the lists of the pair's rows unfilled
    assert got["count"][6] == 0 and (got["tent"][6] == SENT_I32).all()
    assert np.isinf(got["dist"][6, :17]).all() and (got["idx"][6, :17] == -1).all() and (got["dist"][6, 17:] == SENT_F32).all() and (got["idx"][6, 17:] == SENT_I32).all()
    for p in valid:
        r1, n1, r2, n2 = table[p].tolist()
        want = raw_guided(s["D"][r1:r1 + n1], s["D"][r2:r2 + n2], s["L"][r1:r1 + n1], s["L"][r2:r2 + n2], models[p], gf.PLANAR, r, 0.9, True)
        assert 0 < want["count"] < n1, "about a third of the columns are admissible to a row (the float32 restatement keeps 3 rows of either pair)"
        check_guided_pair(got, p, want, n1, p)


# ---- 4. the chains -------------------------------------------------------------------------------------------------------------------------------------
def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _planted_pair(T, seed, rng, epi):
    """Planted frames (planar, or two views of a scene with depth) and descriptors that match along the planted rows."""
    l1, l2, tent, planted = (ep.planted_two_view(T, 0.5, seed)[:4] if epi else sp.planted(T, seed))
    d1, d2 = _unit(rng.normal(size=(T, 128))), rng.normal(size=(T, 128))
    src = np.nonzero(planted)[0]
    d2[tent[src, 1]] = d1[src] + 0.02 * rng.normal(size=(len(src), 128))
    return dev_of(d1), dev_of(l1), dev_of(_unit(d2)), dev_of(l2)


def chain_images(model):
    """Images 0, 1: the repeated scene of 257 rows; 2, 3: a planted pair of 129 rows; 4, 5: of 64; 6, 7: of one row; 8: 300 random rows."""
    if ("chain", model) not in _CACHE:
        epi = model == "fundamental"
        sc = gf.repeated_scene(257, 257, gf.EPIPOLAR if epi else gf.PLANAR)
        descs, lafs = [dev_of(sc["d1"]), dev_of(sc["d2"])], [dev_of(sc["l1"]), dev_of(sc["l2"])]
        rng = np.random.default_rng(5)
        for T, seed in ((129, 2), (64, 3), (1, 4)):
            d1, l1, d2, l2 = _planted_pair(T, seed, rng, epi)
            descs += [d1, d2]
            lafs += [l1, l2]
        descs.append(dev_of(_unit(rng.normal(size=(300, 128)))))
        lafs.append(dev_of(sp.random_frames(rng, 300)))
        _CACHE[("chain", model)] = (descs, lafs, [(0, 1), (2, 3), (4, 5), (6, 7), (0, 8)])
    return _CACHE[("chain", model)]


def _same_result(got, want):
    t1, t2, H, inl, info = got
    w1, w2, wH, winl, winfo = want
    assert torch.equal(t1, w1) and torch.equal(t2, w2) and t1.dtype == torch.int64
    assert torch.equal(H, wH) and H.dtype == torch.float64 and H.shape == (3, 3)
    assert torch.equal(inl, winl) and inl.dtype == torch.bool
    assert torch.equal(info["counts"], winfo["counts"])
    assert {k: v for k, v in info.items() if k != "counts"} == {k: v for k, v in winfo.items() if k != "counts"}


def test_fundamental_chain_equals_the_loop():
    from affnet_amd import ReprojectionStuff as RS
    descs, lafs, pairs = chain_images("fundamental")
    got = RS.match_and_verify_many(descs, lafs, pairs, 0.8, TH, "fundamental", 3, 4, 3)
    assert len(got) == len(pairs)
    for (a, b), g in zip(pairs, got):
        _same_result(g, RS.match_and_verify(descs[a], descs[b], lafs[a], lafs[b], 0.8, TH, "fundamental", 3, rounds=4, seed=3))
    info = got[0][4]
    assert set(info) == {"counts", "best", "best_count", "num_inliers", "flags", "rounds", "seed"} and (info["rounds"], info["seed"]) == (4, 3)
    assert info["flags"] == 0 and info["num_inliers"] >= 8 and info["counts"].numel() == 4 * got[0][0].numel()
    assert got[3][4]["flags"] & 1, "one row: no hypothesis"
    # the default rounds and seed, by keyword, and the tensors of the enqueue form
    _same_result(RS.match_and_verify_many(descs, lafs, pairs[:1], model="fundamental")[0], RS.match_and_verify(descs[0], descs[1], lafs[0], lafs[1], model="fundamental"))
    counts = [int(d.size(0)) for d in descs]
    D, L = torch.cat(descs), torch.cat(lafs)
    out = RS.enqueue_match_and_verify_many(D, L, counts, D, L, counts, pairs, 0.8, TH, "fundamental", 3, 4, 3)
    # cap = the largest n1 of a pair (257), rounds = 4
    assert out[4].shape == (len(pairs), 257 * 4) and out[2].shape == (len(pairs), 3, 3) and out[5].shape == (len(pairs), 4)


@pytest.mark.parametrize("model", ["homography", "affine", "fundamental"])
def test_guided_chain_equals_the_loop(model):
    from affnet_amd import ReprojectionStuff as RS
    descs, lafs, pairs = chain_images(model)
    th = 3.0
    got = RS.match_verify_guided_many(descs, lafs, pairs, 0.8, th, model, rounds=4, seed=3)
    assert len(got) == len(pairs)
    for (a, b), g in zip(pairs, got):
        want = RS.match_verify_guided(descs[a], descs[b], lafs[a], lafs[b], 0.8, th, model, rounds=4, seed=3)
        assert g[4]["seed_stage"] == want[4]["seed_stage"] and set(g[4]["seed_stage"]) == {"tentatives", "num_inliers", "flags"}
        _same_result(g, want)
    print("guided chain %s: %s" % (model, [(g[4]["seed_stage"], g[0].numel(), g[4]["num_inliers"], g[4]["flags"]) for g in got]))
    assert got[0][4]["seed_stage"]["flags"] == 0 and got[0][4]["num_inliers"] >= got[0][4]["seed_stage"]["num_inliers"] > 0
    for mutual in (True, False):
        _same_result(RS.match_verify_guided_many(descs, lafs, pairs[1:2], 0.8, th, model, 0.85, 6.0, mutual, 2)[0],
                     RS.match_verify_guided(descs[2], descs[3], lafs[2], lafs[3], 0.8, th, model, 0.85, 6.0, mutual, 2))


def test_rerank_and_retrieve_under_the_fundamental_model():
    from affnet_amd import ReprojectionStuff as RS
    from affnet_amd import retrieval as R
    descs, lafs, _ = chain_images("fundamental")
    each = {s: RS.match_verify_guided(descs[0], descs[s], lafs[0], lafs[s], 0.8, TH, "fundamental") for s in (8, 1)}
    order, num = RS.spatial_rerank(descs, lafs, 0, [8, 1], 0.8, TH, "fundamental", guided=True)
    assert order == [1, 8] and num == [each[1][4]["num_inliers"], each[8][4]["num_inliers"]] and num[0] >= 8 and num[0] > num[1]
    plain = {s: RS.match_and_verify(descs[0], descs[s], lafs[0], lafs[s], 0.8, TH, "fundamental", rounds=2, seed=1)[4]["num_inliers"] for s in (8, 1)}
    assert RS.spatial_rerank(descs, lafs, 0, [8, 1], 0.8, TH, "fundamental", rounds=2, seed=1) == ([1, 8], [plain[1], plain[8]])
    assert RS.spatial_rerank(descs, lafs, 0, [], model="fundamental", guided=True) == ([], [])
    index = R.DescriptorIndex(descs, lafs)
    res = index.retrieve(descs[0], lafs[0], top=3, exclude=0, inl_th=TH, model="fundamental", guided=True)
    assert res and res[0]["image"] == 1 and [e["num_inliers"] for e in res] == sorted((e["num_inliers"] for e in res), reverse=True)
    for e in res:
        t1, t2, F, inl, info = RS.match_verify_guided(descs[0], descs[e["image"]], lafs[0], lafs[e["image"]], 0.8, TH, "fundamental")
        assert torch.equal(e["tent_in_1"], t1) and torch.equal(e["tent_in_2"], t2) and torch.equal(e["H"], F) and torch.equal(e["inliers"], inl)
        assert e["num_inliers"] == info["num_inliers"] and e["seed_stage"] == info["seed_stage"]
    plain = index.retrieve(descs[0], lafs[0], top=3, exclude=0, inl_th=TH, model="fundamental", rounds=2, seed=1)
    for e in plain:
        t1, t2, F, inl, info = RS.match_and_verify(descs[0], descs[e["image"]], lafs[0], lafs[e["image"]], 0.8, TH, "fundamental", rounds=2, seed=1)
        assert torch.equal(e["tent_in_1"], t1) and torch.equal(e["H"], F) and torch.equal(e["inliers"], inl) and "seed_stage" not in e


# ---- 5. the single-pair entry points after the batched calls ----------------------------------------------------------------------------------------
def test_single_pair_calls_keep_their_bytes(recorded_single_pair_calls):
    """The last test of the module: the batched calls of every test in front of it lie between the two recordings."""
    e, g = epi_set(), guided_set()
    raw_epi_many(e["L1"], e["L2"], e["table"], e["d_tent"], e["d_count"], e["t_max"], 8, 3)
    raw_guided_many(g["D1"], g["D2"], g["L1"], g["L2"], g["table"], g["n1_max"], g["n2_max"], guided_models(gf.PLANAR), gf.PLANAR, gf.DENSE_R, 0.9, True)
    v0, m0 = recorded_single_pair_calls
    v, m = _recorded_calls()
    assert all(same(v[k], v0[k]) for k in v) and v["summary"][3] == 0
    assert m["count"] == m0["count"] > 0 and all(same(m[k], m0[k]) for k in ("dist", "idx", "tent"))
