"""MI355X: the single-pair matcher (affnet_amd/csrc/match.hip: affnet_distance_matrix, affnet_match_snn, and their Python callers) against
its float32 restatement tests/_match_fp32.py, which tests/test_match_mirror_host.py pins to libm fmaf, the oracle and the golden pair.  Every
other matching test of the suite (the batched matcher, the descriptor index, the inverted file) compares with these two calls, so they are
compared here with something that is not the device: every comparison below is on the bytes (NaN distances by their bit pattern), at the
sizes one below, at and one above the 16-row wave, the 16-column tile, the 64-row workgroup and the 1024-row selection round, on inputs with
exact ties, NaN rows, unused columns and kept and refused rows (the host test asserts that they are there).

The restatement rests on one v_mfma_f32_16x16x4_f32 being the K-ordered fmaf chain with one rounding per product; the first test of this
file checks exactly that on an input that tells the 24 orders and the unfused form apart."""
import numpy as np
import pytest
import torch

import _match_fp32 as mf
import test_gpu_match_many as mm
from _fp32_chain import F32

pytestmark = pytest.mark.gpu

DEV = mm.DEV
SENT_F32, SENT_I32, SENT_U8 = mm.SENT_F32, mm.SENT_I32, mm.SENT_U8
same = mm.same
THR = 0.8
GUARD = 256         # sentinel bytes behind the scratch buffer, sentinel elements behind the matrix


def dev(x):
    return torch.tensor(np.ascontiguousarray(x)).to(DEV)          # a copy: the planted arrays are read-only


_DEVICE = {}


def planted_dev(n1, n2):
    if (n1, n2) not in _DEVICE:
        q, db = mf.planted(n1, n2)
        _DEVICE[(n1, n2)] = (dev(q), dev(db))
    return _DEVICE[(n1, n2)]


def guarded_scratch(nbytes):
    return mm.full((nbytes + GUARD,), SENT_U8, torch.uint8)


def guard_intact(scratch, nbytes):
    return bool((scratch[nbytes:] == SENT_U8).all()) and scratch.numel() == nbytes + GUARD


def hexs(x):
    return ["%08x" % v for v in np.ascontiguousarray(x, F32).view(np.uint32).ravel().tolist()]


def describe(name, got, want, limit=8):
    """The first differing elements, for the assertion message."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "%s: %s %s against %s %s" % (name, got.shape, got.dtype, want.shape, want.dtype)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel()) if got.dtype.itemsize == 4 else np.flatnonzero(got.ravel() != want.ravel())
    rows = ["[%s] got %r want %r" % (",".join(map(str, np.unravel_index(i, got.shape))), got.ravel()[i], want.ravel()[i]) for i in bad[:limit]]
    return "%s: %d of %d elements differ: %s" % (name, bad.size, got.size, "; ".join(rows))


def test_one_mfma_is_the_k_ordered_fmaf_chain():
    lib, ptr, check, ctx, st, d = mm._api()
    A, B = mf.mfma_input()
    dA, dB, out = dev(A), dev(B), mm.full((16 * 16 + 64,), SENT_F32, torch.float32)
    assert lib.affnet_selftest_mfma(ptr(dA), ptr(dB), ptr(out), st) == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[256:] == SENT_F32).all()
    got, want = out[:256].reshape(16, 16), mf.mfma_chain(A, B)
    if not same(got, want):       # which form the device does compute, if any of those the host test tells apart
        forms = [str(o) for o in mf.K_ORDERS if same(got, mf.mfma_chain(A, B, o))] + (["unfused"] if same(got, mf.mfma_unfused(A, B)) else [])
        print("the device's tile equals: %s" % (forms or "none of the 24 chain orders, nor the unfused sum"))
    assert same(got, want), describe("one MFMA against fma(a3,b3, fma(a2,b2, fma(a1,b1, fma(a0,b0, 0))))", got, want)


def raw_matrix_guarded(q, db, n1, n2):
    lib, ptr, check, ctx, st, d = mm._api()
    out = mm.full((n1 * n2 + GUARD,), SENT_F32, torch.float32)
    nb = lib.affnet_match_scratch_bytes(n1, n2)
    scratch = guarded_scratch(nb)
    check(lib.affnet_distance_matrix(ctx, ptr(q), n1, ptr(db), n2, 128, ptr(out), ptr(scratch), st), ctx, "affnet_distance_matrix")
    out = out.cpu().numpy()
    assert guard_intact(scratch, nb), "affnet_distance_matrix wrote behind affnet_match_scratch_bytes"
    assert (out[n1 * n2:] == SENT_F32).all(), "affnet_distance_matrix wrote behind the n1 x n2 matrix"
    return out[:n1 * n2].reshape(n1, n2)


@pytest.mark.parametrize("n1,n2", mf.MATRIX_SHAPES)
def test_distance_matrix(n1, n2):
    q, db = planted_dev(n1, n2)
    want = mf.planted_mirror(n1, n2)["M"]
    got = raw_matrix_guarded(q, db, n1, n2)
    nan = np.isnan(want)
    if nan.any():
        print("%d x %d: %d NaN distances, the device's bit patterns %s, numpy's %s" % (n1, n2, nan.sum(), sorted(set(hexs(got[nan]))), sorted(set(hexs(want[nan])))))
    assert same(got, want), describe("distance matrix %d x %d" % (n1, n2), got, want)


def test_distance_matrix_without_rows_or_columns_writes_nothing():
    q, db = planted_dev(17, 33)
    lib, ptr, check, ctx, st, d = mm._api()
    out, scratch = mm.full((17 * 33,), SENT_F32, torch.float32), guarded_scratch(0)
    for n1, n2 in ((0, 33), (17, 0), (0, 0)):
        check(lib.affnet_distance_matrix(ctx, ptr(q), n1, ptr(db), n2, 128, ptr(out), ptr(scratch), st), ctx, "affnet_distance_matrix")
    torch.cuda.synchronize()
    assert bool((out == SENT_F32).all()) and guard_intact(scratch, 0)


def test_losses_distance_matrix_vector_is_the_same_call():
    from affnet_amd import Losses
    q, db = planted_dev(65, 200)
    got = Losses.distance_matrix_vector(q, db)
    assert got.shape == (65, 200) and got.dtype == torch.float32
    assert same(got.cpu().numpy(), mf.planted_mirror(65, 200)["M"])
    assert Losses.distance_matrix_vector(q[:0], db).shape == (0, 200)


def raw_snn_guarded(d1, d2, n1, n2, thr):
    """affnet_match_snn like test_gpu_match_many.raw_snn, on a scratch buffer of exactly affnet_match_scratch_bytes bytes with sentinels behind."""
    lib, ptr, check, ctx, st, d = mm._api()
    rows = max(n1, 1)
    md, md2, idx = mm.full((rows,), SENT_F32, torch.float32), mm.full((rows,), SENT_F32, torch.float32), mm.full((rows,), SENT_I32, torch.int32)
    tent, cnt = mm.full((rows, 2), SENT_I32, torch.int32), mm.full((1,), SENT_I32, torch.int32)
    nb = lib.affnet_match_scratch_bytes(n1, n2)
    scratch = guarded_scratch(nb)
    check(lib.affnet_match_snn(ctx, ptr(d1), n1, ptr(d2), n2, 128, thr, ptr(md), ptr(idx), ptr(md2), ptr(tent), ptr(cnt), ptr(scratch), st), ctx, "affnet_match_snn")
    out = dict(md=md.cpu().numpy(), idx=idx.cpu().numpy(), md2=md2.cpu().numpy(), tent=tent.cpu().numpy(), count=int(cnt.item()))
    assert guard_intact(scratch, nb), "affnet_match_snn wrote behind affnet_match_scratch_bytes"
    return out


def assert_is_the_mirror(got, want, what):
    """md, idx, md2, count, tent[:count] on the bytes; the rows of tent at and beyond the count untouched."""
    for name in ("md", "idx", "md2"):
        assert same(got[name], want[name]), describe("%s %s" % (what, name), got[name], want[name])
    k = want["count"]
    assert got["count"] == k, "%s: count %d, the mirror's %d" % (what, got["count"], k)
    assert same(got["tent"][:k], want["tent"]), describe("%s tentatives" % (what,), got["tent"][:k], want["tent"])
    assert (got["tent"][k:] == SENT_I32).all(), "%s: rows at or beyond the count are written" % (what,)


@pytest.mark.parametrize("n1,n2", mf.MATCH_SHAPES)
def test_matcher(n1, n2):
    q, db = planted_dev(n1, n2)
    want = mf.planted_mirror(n1, n2, THR)
    got = raw_snn_guarded(q, db, n1, n2, THR)
    assert_is_the_mirror(got, want, "%d x %d" % (n1, n2))
    again = mm.raw_snn(q, db, THR)
    assert again["count"] == got["count"] and all(same(again[k], got[k]) for k in ("md", "idx", "md2", "tent")), "a second call gives other bytes"


def test_match_snn_wrapper_returns_the_same_values():
    from affnet_amd import ReprojectionStuff as RS
    q, db = planted_dev(65, 200)
    want = mf.planted_mirror(65, 200, THR)
    t1, t2, md, md2 = RS.match_snn(q, db, THR)
    assert t1.dtype == torch.int64 and t2.dtype == torch.int64
    assert np.array_equal(t1.cpu().numpy(), want["tent"][:, 0]) and np.array_equal(t2.cpu().numpy(), want["tent"][:, 1])
    assert same(md.cpu().numpy(), want["md"]) and same(md2.cpu().numpy(), want["md2"])


def test_no_query_rows():
    q, db = planted_dev(17, 33)
    got = raw_snn_guarded(q, db, 0, 33, THR)
    assert got["count"] == 0
    assert (got["md"] == SENT_F32).all() and (got["md2"] == SENT_F32).all() and (got["idx"] == SENT_I32).all() and (got["tent"] == SENT_I32).all()


@pytest.mark.parametrize("n1,n2", [(65, 200), (2049, 200)])
def test_thresholds(n1, n2):
    q, db = planted_dev(n1, n2)
    base = mf.planted_mirror(n1, n2, THR)
    M = base["M"]
    ok = base["keep"] & np.isfinite(base["ratio"]) & (base["ratio"] > 0)
    r = int(np.nonzero(ok)[0][np.argmax(base["ratio"][ok])])          # the kept row with the largest finite ratio
    at = float(base["ratio"][r])
    below = float(np.nextafter(F32(at), F32(-np.inf)))
    for thr, row_kept in ((at, True), (below, False), (0.0, None), (float("inf"), None)):
        want = mf.match_from_matrix(M, thr)
        got = mm.raw_snn(q, db, thr)
        assert_is_the_mirror(got, want, "%d x %d at threshold %r" % (n1, n2, thr))
        if row_kept is not None:
            assert (r in got["tent"][:got["count"], 0].tolist()) == row_kept, "row %d with ratio %r at threshold %r" % (r, at, thr)
        if thr == float("inf"):
            assert got["count"] == int((~np.isnan(base["ratio"])).sum()) < n1, "every row whose ratio is a number, and the NaN rows are not"
        if thr == 0.0:
            assert got["count"] == want["count"] == int((base["ratio"] <= 0).sum())


def test_batched_pairs_across_a_selection_round():
    from affnet_amd import ReprojectionStuff as RS
    shapes = [(1025, 200), (65, 200), (17, 33)]
    D1 = torch.cat([planted_dev(*s)[0] for s in shapes])
    D2 = torch.cat([planted_dev(*s)[1] for s in shapes])
    table, n1_max, n2_max = RS.pair_table([s[0] for s in shapes], [s[1] for s in shapes], [(0, 0), (1, 1), (2, 2)])
    assert (n1_max, n2_max) == (1025, 200)
    got = mm.raw_snn_many(D1, D2, table, n1_max, n2_max, THR)
    for p, (n1, n2) in enumerate(shapes):
        want = mf.planted_mirror(n1, n2, THR)
        pair = dict(md=got["md"][p, :n1], idx=got["idx"][p, :n1], md2=got["md2"][p, :n1], tent=got["tent"][p], count=int(got["count"][p]))
        assert_is_the_mirror(pair, want, "pair %d (%d x %d)" % (p, n1, n2))
        assert (got["md"][p, n1:] == SENT_F32).all() and (got["md2"][p, n1:] == SENT_F32).all() and (got["idx"][p, n1:] == SENT_I32).all(), "rows n1 .. n1_max"
