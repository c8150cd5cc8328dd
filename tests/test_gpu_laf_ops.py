"""Unit sweep of the elementwise kernels of csrc/laf_ops.hip (shape_filter_kernel / aff_shape_filter_row, shape_iterate_kernel,
apply_rotation_kernel, scale_lafs_kernel, level_select_kernel, lafs2ell_kernel) and csrc/match.hip (reproject_lafs_kernel,
centre_nn_kernel) against the exact fp32 mirrors of tests/_laf_mirror.py: row counts around the 256-thread block edge, a ragged batch of
three images, planted rows next to every threshold, and sentinel-filled output buffers that pin what each kernel does with the rows at
or past its count (some zero them, some leave them alone).  Comparisons are bit for bit unless stated; tests/test_laf_mirror_host.py
pins the mirrors to the oracle and checks the fixtures' margins on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _laf_mirror as lm
from _fp32_chain import F32
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 777.0
ISENT = -777
ROWS = [1, 255, 256, 257]
CAP = 300
BATCH_COUNTS = (0, 1, 257)
H, W = 64, 80


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return affnet_amd


@pytest.fixture(scope="module")
def ctxs(amd):
    """Contexts of one and of three 64 x 80 images, three levels, capacity 300 before and after the shape filter (num_features >= every row
    count: the selection is the stable compaction of the good rows)."""
    from affnet_amd import engine
    mk = lambda b: engine.Context(H, W, torch.device(DEV), 3, 1.6, 5, 5.192, 0.0, CAP, CAP, batch=b)
    c1, c3 = mk(1), mk(3)
    assert c1.cap_pre == c1.cap_final == c3.cap_pre == c3.cap_final == CAP and c3.batch == 3
    return {1: c1, 3: c3}


def _st():
    from affnet_amd import engine
    return engine.stream_of(torch.device(DEV))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cnt(counts):
    return torch.tensor(list(counts), dtype=torch.int32, device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy()


def _eq(got, want):
    """Bit-for-bit equality of float arrays (NaN rows included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.int32) if got.dtype == F32 else got,
                                                                                  want.view(np.int32) if want.dtype == F32 else want)


def _cases():
    """(context key, n_max, counts or None) for every row count: no count pointer, a count pointer, and the ragged batch."""
    out = [(1, n, None) for n in ROWS] + [(1, CAP, (n,)) for n in ROWS] + [(3, CAP, BATCH_COUNTS)]
    return out


def _tile(a, b, n_max):
    """Rows of a per-image array for b images of n_max rows each: image i starts i * 7 rows into the (cyclic) fixture."""
    return np.stack([np.roll(a, -7 * i, axis=0)[:n_max] for i in range(b)])


# ---- shape filter ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_fix():
    rows = lm.shape_rows(CAP)
    fig = lm.shape_rows_conditions(*rows)                  # no ambiguous row; accepted and rejected rows for each criterion (asserted inside)
    return rows, fig


@pytest.mark.parametrize("case", [(1, (n,)) for n in ROWS] + [(3, BATCH_COUNTS)], ids=lambda c: "b%d-%s" % (c[0], "-".join(map(str, c[1]))))
def test_shape_filter_select(amd, ctxs, shape_fix, case):
    from affnet_amd._lib import lib, check, ptr
    (resp, L, ids, A, grp), fig = shape_fix
    b, counts = case
    ctx = ctxs[b]
    r, l, i, a = (_tile(x, b, CAP) for x in (resp, L, ids, A))
    dr, dl, di, da, dc = _dev(r), _dev(l), _dev(i), _dev(a), _cnt(counts)
    r2 = torch.full((b, CAP), SENT, device=DEV); l2 = torch.full((b, CAP, 2, 3), SENT, device=DEV)
    i2 = torch.full((b, CAP, 3), ISENT, dtype=torch.int32, device=DEV); c2 = torch.full((b,), ISENT, dtype=torch.int32, device=DEV)
    check(lib.affnet_shape_filter_select(ctx.handle, ptr(dr), ptr(dl), ptr(di), ptr(da), ptr(dc), ptr(r2), ptr(l2), ptr(i2), ptr(c2), _st()), ctx.handle,
          "affnet_shape_filter_select")
    torch.cuda.synchronize()
    r2, l2, i2, c2 = _bits(r2), _bits(l2), _bits(i2), _bits(c2)
    kept = []
    for k, n in enumerate(counts):
        wr, wl, wi = lm.shape_filter_select(r[k], l[k], i[k], a[k], n, CAP)
        m = len(wr)
        kept.append(m)
        assert int(c2[k]) == m, (k, n, int(c2[k]), m)
        assert np.array_equal(i2[k, :m], wi), "image %d: not the mirror's surviving rows in input order" % k
        assert _eq(r2[k, :m], wr) and _eq(l2[k, :m], wl), "image %d: responses or composed frames differ from the mirror" % k
        assert not r2[k, m:].any() and not l2[k, m:].any() and not i2[k, m:].any()              # rows past the output count: zero
    if sum(counts) >= 255:
        assert 0 < max(kept) < max(counts)
    record_parity("shape filter vs mirror, counts %s" % (counts,), kept=kept, **fig)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", [(1, (n,)) for n in ROWS] + [(3, BATCH_COUNTS)], ids=lambda c: "b%d-%s" % (c[0], "-".join(map(str, c[1]))))
def test_shape_iterate(amd, ctxs, shape_fix, case, mode):
    from affnet_amd._lib import lib, check, ptr
    (resp, L, ids, A, grp), _ = shape_fix
    b, counts = case
    ctx = ctxs[b]
    rng = np.random.RandomState(31)
    base = (np.eye(2).reshape(1, 4) + rng.normal(0.0, 0.5, (CAP, 4))).astype(F32)
    a, bs, l = _tile(A, b, CAP), _tile(base, b, CAP), _tile(L, b, CAP)
    da, db, dl, dc = _dev(a), _dev(bs), _dev(l), _cnt(counts)
    out = torch.full((b, CAP, 2, 3), SENT, device=DEV)
    check(lib.affnet_shape_iterate(ctx.handle, ptr(da) if mode else None, ptr(db), ptr(dl), ptr(dc), mode, ptr(out), _st()), ctx.handle, "affnet_shape_iterate")
    torch.cuda.synchronize()
    gb, go = _bits(db), _bits(out)
    for k, n in enumerate(counts):
        wb, wo = lm.shape_iterate(a[k, :n], bs[k, :n], l[k, :n], mode)
        assert _eq(gb[k, :n], wb) and _eq(go[k, :n], wo), (k, n)
        assert _eq(gb[k, n:], bs[k, n:]) and np.all(go[k, n:] == SENT)                          # rows at or past the count: untouched
    if mode == 0:
        assert _eq(gb, bs)
    else:
        assert max(counts) == 1 or not _eq(gb, bs)


# ---- apply_rotation / scale_lafs ------------------------------------------------------------------------------------------------------------
def _case_id(c):
    return "b%d-n%d-%s" % (c[0], c[1], "all" if c[2] is None else "-".join(map(str, c[2])))


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_apply_rotation(amd, ctxs, shape_fix, case):
    from affnet_amd._lib import lib, check, ptr
    (_, L, _, _, _), _ = shape_fix
    b, n_max, counts = case
    ctx = ctxs[b]
    rng = np.random.RandomState(32)
    ang = rng.uniform(-np.pi, np.pi, CAP)
    R = np.stack([np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)], axis=1).astype(F32)
    R[::17] = (np.eye(2).reshape(1, 4) + rng.normal(0, 0.3, (len(R[::17]), 4))).astype(F32)      # not only rotations: any 2x2 factor
    l, r = _tile(L, b, n_max), _tile(R, b, n_max)
    buf = torch.full((b * n_max + 1, 2, 3), SENT, device=DEV)                                   # one row more than the kernel may touch
    buf[:b * n_max] = _dev(l).view(-1, 2, 3)
    dr = _dev(r)
    dc = None if counts is None else _cnt(counts)
    check(lib.affnet_apply_rotation(ctx.handle, ptr(buf), ptr(dr), ptr(dc), n_max, _st()), ctx.handle, "affnet_apply_rotation")
    torch.cuda.synchronize()
    got = _bits(buf)
    assert np.all(got[-1] == SENT)
    got = got[:-1].reshape(b, n_max, 2, 3)
    for k in range(b):
        n = n_max if counts is None else counts[k]
        assert _eq(got[k, :n], lm.apply_rotation(l[k, :n], r[k, :n])), (k, n)
        assert _eq(got[k, n:], l[k, n:])                                                         # rows at or past the count: untouched


@pytest.mark.parametrize("wh", [(80, 64), (64, 80), (641, 481)])
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_scale_lafs(amd, ctxs, shape_fix, case, inverse, wh):
    from affnet_amd._lib import lib, check, ptr
    (_, L, _, _, _), _ = shape_fix
    b, n_max, counts = case
    ctx = ctxs[b]
    w, h = wh
    src = lm.scale_lafs(L, w, h, False) if inverse else L                                       # pixel frames in for the inverse direction
    l = _tile(src, b, n_max)
    out = torch.full((b * n_max + 1, 2, 3), SENT, device=DEV)
    dl = _dev(l)
    dc = None if counts is None else _cnt(counts)
    check(lib.affnet_scale_lafs(ctx.handle, ptr(dl), ptr(out), ptr(dc), n_max, w, h, inverse, _st()), ctx.handle,
          "affnet_scale_lafs")
    torch.cuda.synchronize()
    got = _bits(out)
    assert np.all(got[-1] == SENT)
    got = got[:-1].reshape(b, n_max, 2, 3)
    for k in range(b):
        n = n_max if counts is None else counts[k]
        assert _eq(got[k, :n], lm.scale_lafs(l[k, :n], w, h, bool(inverse))), (k, n)
        assert not got[k, n:].any()                                                              # rows at or past the count: zero


# ---- level_select ---------------------------------------------------------------------------------------------------------------------------
def _sigmas(ctx):
    cfg = ctx.cfg
    return np.array([[cfg.level_sigma_px[o][l] for l in range(cfg.levels_per_octave)] for o in range(cfg.n_octaves)])


@pytest.mark.parametrize("ps", [32, 19])
def test_level_select(amd, ctxs, ps):
    from affnet_amd._lib import lib, check, ptr
    sig2 = _sigmas(ctxs[1])
    n_oct, n_lvl = sig2.shape
    assert n_lvl == 5 and n_oct >= 2 and np.array_equal(sig2, _sigmas(ctxs[3]))                # three levels (+ 2), at least two octaves
    sig = sig2.reshape(-1)
    twins = [(i, j) for i in range(sig.size) for j in range(i + 1, sig.size) if sig[i] == sig[j] and i // n_lvl != j // n_lvl]
    assert twins, "the level table holds no pair of exactly equal sigmas in different octaves"
    F, T, K = lm.level_frames(sig, ps, CAP)
    mg = lm.level_margin(F, ps, sig)
    assert np.nanmin(mg[K != "nan"]) > 1e-6
    want_best, _ = lm.level_argmin(F, ps, sig)
    # rows on or near an equal pair must resolve to the lower (octave, level): stated here from the table, not from the mirror
    hits = 0
    for i, j in twins:
        with np.errstate(invalid="ignore"):
            sel = np.isin(K, ("on", "near")) & (np.abs(T / sig[i] - 1.0) < 2e-3)
        assert sel.sum() >= 6 and np.all(want_best[sel] == i) and not np.any(want_best == j)
        hits += int(sel.sum())
    nan_row = int(np.nonzero(K == "nan")[0][0])
    assert want_best[nan_row] == 0
    chosen = set()
    for b, n_max, counts in _cases():
        ctx = ctxs[b]
        f = _tile(F, b, n_max)
        ids = torch.full((b * n_max + 1, 3), ISENT, dtype=torch.int32, device=DEV)
        norm = torch.full((b * n_max + 1, 2, 3), SENT, device=DEV)
        df = _dev(f)
        dc = None if counts is None else _cnt(counts)
        check(lib.affnet_level_select(ctx.handle, ptr(df), ptr(dc), n_max, ps, ptr(ids), ptr(norm), _st()), ctx.handle,
              "affnet_level_select")
        torch.cuda.synchronize()
        gi, gn = _bits(ids), _bits(norm)
        assert np.all(gi[-1] == ISENT) and np.all(gn[-1] == SENT)
        gi, gn = gi[:-1].reshape(b, n_max, 3), gn[:-1].reshape(b, n_max, 2, 3)
        for k in range(b):
            n = n_max if counts is None else counts[k]
            wi, wn = lm.level_select(f[k, :n], ps, sig, n_lvl, W, H)
            bad = np.nonzero((gi[k, :n] != wi).any(axis=1))[0]
            assert bad.size == 0, "case %s image %d: rows %s got %s, the mirror %s (kinds %s)" % ((b, n_max, counts), k, bad[:8].tolist(), gi[k, bad[:8]].tolist(),
                                                                                                   wi[bad[:8]].tolist(), np.roll(K, -7 * k)[bad[:8]].tolist())
            assert _eq(gn[k, :n], wn), (b, n_max, counts, k)
            assert np.all(gi[k, n:] == ISENT) and np.all(gn[k, n:] == SENT)                     # rows at or past the count: untouched
            chosen |= set(map(tuple, gi[k, :n, :2].tolist()))
        if b == 1 and n_max >= 257 and counts is None:
            assert gi[0, nan_row].tolist() == [0, 0, 0]                                         # the NaN frame: level (0, 0)
            for i, j in twins:
                assert (j // n_lvl, j % n_lvl) not in set(map(tuple, gi[0, :, :2].tolist()))
    record_parity("level_select vs mirror, ps %d" % ps, equal_sigma_pairs=len(twins), rows_on_equal_sigmas=hits, levels_chosen=len(chosen),
                  smallest_margin=float(np.nanmin(mg[K != "nan"])))
    assert len(chosen) >= 10


# ---- lafs_to_ellipses -----------------------------------------------------------------------------------------------------------------------
def test_lafs_to_ellipses(amd, ctxs):
    from affnet_amd._lib import lib, check, ptr
    frames, kind = lm.ellipse_frames()
    e_ref, _, want = lm.ellipse_reference_error(frames, kind)
    rng = np.random.RandomState(9)
    order = rng.permutation(len(frames))
    frames, kind, want = np.concatenate([frames[order]] * 2)[:CAP], np.concatenate([kind[order]] * 2)[:CAP], np.concatenate([want[order]] * 2)[:CAP]
    assert {"aniso", "iso", "negdet", "zero"} <= set(kind[:255].tolist())
    worst = {"aniso": 0.0, "iso": 0.0}
    for b, n_max, counts in _cases():
        ctx = ctxs[b]
        f = _tile(frames, b, n_max)
        out = torch.full((b * n_max + 1, 5), SENT, device=DEV)
        df = _dev(f)
        dc = None if counts is None else _cnt(counts)
        check(lib.affnet_lafs_to_ellipses(ctx.handle, ptr(df), ptr(dc), n_max, ptr(out), _st()), ctx.handle,
              "affnet_lafs_to_ellipses")
        torch.cuda.synchronize()
        got = _bits(out)
        assert np.all(got[-1] == SENT)
        got = got[:-1].reshape(b, n_max, 5)
        for k in range(b):
            n = n_max if counts is None else counts[k]
            kd, wt = np.roll(kind, -7 * k)[:n], np.roll(want, -7 * k, axis=0)[:n]
            assert not got[k, n:].any()                                                          # rows at or past the count: zero
            assert _eq(got[k, :n, :2], np.ascontiguousarray(f[k, :n, :, 2]))                    # the two centre columns: exact, every kind
            assert np.array_equal(np.isfinite(got[k, :n]), np.isfinite(wt)), "non-finite pattern differs from the restatement"
            err = lm.ellipse_rel_err(got[k, :n], wt)
            for name in worst:
                if (kd == name).any():
                    worst[name] = max(worst[name], float(err[kd == name].max()))
    print("lafs_to_ellipses: worst relative error %s, reference's own %s, bar 8 x" % (worst, e_ref))
    record_parity("lafs_to_ellipses vs float64 restatement", **{"err_" + k: v for k, v in worst.items()}, **{"bar_" + k: 8.0 * v for k, v in e_ref.items()})
    for name in worst:
        assert worst[name] <= 8.0 * e_ref[name], (name, worst[name], e_ref[name])


# ---- reproject_lafs / centre_nn -------------------------------------------------------------------------------------------------------------
def _homographies(golden_dir):
    Hg = np.load(os.path.join(golden_dir, "match_graf16_n500.npz"))["H"].astype(F32)
    sim = np.array([[0.8 * np.cos(0.4), -0.8 * np.sin(0.4), 31.5], [0.8 * np.sin(0.4), 0.8 * np.cos(0.4), -12.25], [0.0, 0.0, 1.0]])
    return [("graf 1-6", Hg), ("graf 6-1", np.linalg.inv(Hg.astype(np.float64)).astype(F32)), ("identity", np.eye(3, dtype=F32)), ("similarity", sim.astype(F32))]


@pytest.mark.parametrize("n", ROWS)
def test_reproject_lafs(amd, ctxs, golden_dir, n):
    """Exact against the mirror: the kernel's divisions (h / den, X / Z) must be correctly rounded fp32 divisions for this to hold."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, check, ptr
    L = np.load(os.path.join(golden_dir, "match_graf16_n500.npz"))["LAFs2"].astype(F32)[:n]
    ctx = engine.utility_ctx(torch.device(DEV))
    dl = _dev(L)
    for name, Hm in _homographies(golden_dir):
        out = torch.full((n + 1, 2, 3), SENT, device=DEV)
        h9 = (C.c_float * 9)(*[float(v) for v in Hm.reshape(-1)])
        check(lib.affnet_reproject_lafs(ctx, ptr(dl), n, h9, ptr(out), _st()), ctx, "affnet_reproject_lafs")
        torch.cuda.synchronize()
        got = _bits(out)
        want = lm.reproject_lafs(L, Hm)
        assert np.all(got[n] == SENT)
        d = np.abs(got[:n].astype(np.float64) - want)
        assert _eq(got[:n], want), "%s: %d of %d entries differ from the mirror, worst %.3g" % (name, int((got[:n] != want).sum()), want.size, d.max())
        if name == "identity":
            assert _eq(got[:n], L)


@pytest.mark.parametrize("nr", [1, 2, 300])
@pytest.mark.parametrize("nq", [1, 127, 128, 129])
def test_centre_nn(amd, ctxs, nq, nr):
    from affnet_amd import engine
    from affnet_amd._lib import lib, check, ptr
    rng = np.random.RandomState(1000 * nq + nr)
    q, r = np.zeros((nq, 2, 3), dtype=F32), np.zeros((nr, 2, 3), dtype=F32)
    q[:, :, :2], r[:, :, :2] = rng.normal(0, 9, (nq, 2, 2)), rng.normal(0, 9, (nr, 2, 2))        # the 2x2 parts must not matter
    r[:, :, 2] = rng.uniform(760.0, 840.0, (nr, 2))
    q[:, :, 2] = r[rng.randint(0, nr, nq), :, 2] + rng.normal(0.0, 2.0, (nq, 2))                # ~800 px: the expansion cancels heavily
    if nr >= 2:
        r[nr // 2:] = r[:nr - nr // 2]                                                           # exact duplicates: the first index must win
        q[0, :, 2] = r[0, :, 2]
    ctx = engine.utility_ctx(torch.device(DEV))
    md = torch.full((nq + 1,), SENT, device=DEV)
    idx = torch.full((nq + 1,), ISENT, dtype=torch.int32, device=DEV)
    dq, dr = _dev(q), _dev(r)
    check(lib.affnet_centre_nn(ctx, ptr(dq), nq, ptr(dr), nr, ptr(md), ptr(idx), _st()), ctx, "affnet_centre_nn")
    torch.cuda.synchronize()
    gm, gi = _bits(md), _bits(idx)
    wm, wi = lm.centre_nn(q, r)
    assert float(gm[nq]) == SENT and int(gi[nq]) == ISENT
    assert np.array_equal(gi[:nq], wi), "rows %s" % np.nonzero(gi[:nq] != wi)[0][:8].tolist()
    assert _eq(gm[:nq], wm)
    if nr >= 2:
        assert np.all(gi[:nq] < nr - nr // 2)                                                    # never the later copy of a duplicated centre
