"""Pins every mirror of tests/_laf_mirror.py to the oracle's torch function of the same operation on random inputs (CPU), so that
tests/test_gpu_laf_ops.py compares the kernels with something the project already trusts.  Elementwise chains must agree bit for bit;
where the oracle goes through torch.bmm - whose CPU kernel may or may not fuse the accumulate - the mirror must be the fused chain exactly
or lie within the rounding of the unfused one, and the worst difference is recorded."""
import numpy as np
import pytest
import torch

import _laf_mirror as lm
import affnet_oracle as orc
from _fp32_chain import F32
from conftest import record_parity

EPS = float(np.finfo(np.float32).eps)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rand_lafs(rng, n, scale=0.05, lo=0.2, hi=0.8):
    L = np.empty((n, 2, 3), dtype=F32)
    L[:, :, :2] = rng.normal(0.0, scale, (n, 2, 2))
    L[:, :, 2] = rng.uniform(lo, hi, (n, 2))
    return L


def _rand_A(rng, n):
    return (np.eye(2)[None] + rng.normal(0.0, 0.6, (n, 2, 2))).astype(F32)


def _bmm_check(name, got, want, bound):
    """got = the mirror's fused chain, want = torch.bmm: equal, or within `bound` (the rounding of the products the two forms round
    differently)."""
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    exact = bool(np.array_equal(got, want))
    worst = float((d / bound).max())
    record_parity("LAF mirror vs torch.bmm (host): " + name, bit_identical=exact, worst_difference=float(d.max()), worst_over_bound=worst)
    print("%s: %s, worst difference %.3g (%.3g of the bound)" % (name, "bit-identical" if exact else "torch.bmm is not the fused chain here", d.max(), worst))
    assert worst <= 1.0, name
    return exact


def test_eig2x2_and_inside_image():
    rng = np.random.RandomState(1)
    A, L = _rand_A(rng, 4000), _rand_lafs(rng, 4000, scale=0.12)
    l1, l2, d1 = lm.eig2x2(A.reshape(-1, 4))
    w1, w2 = orc.eig2x2(_t(A))
    # torch's CPU sqrt is not correctly rounded on every host (numpy's and the device's sqrtf are): with torch's root handed to the mirror
    # every operation agrees bit for bit; with the correctly rounded one the eigenvalues move by at most that one ulp of the root
    t1, t2, _ = lm.eig2x2(A.reshape(-1, 4), sqrt=lambda v: torch.sqrt(_t(v)).numpy())
    assert np.array_equal(t1, w1.numpy()) and np.array_equal(t2, w2.numpy())
    root = np.sqrt(np.abs(d1.astype(np.float64)))
    worst = max(np.abs(l1.astype(np.float64) - w1.numpy()).max(), np.abs(l2.astype(np.float64) - w2.numpy()).max())
    record_parity("LAF mirror vs orc.eig2x2 (host)", rows_differing=int(((l1 != w1.numpy()) | (l2 != w2.numpy())).sum()), worst_difference=float(worst))
    bound = EPS * (np.abs(A[:, 0, 0].astype(np.float64) + A[:, 1, 1]) + 2.0 * root)          # one ulp of the root, then one rounding of tr +- root
    assert (np.abs(l1.astype(np.float64) - w1.numpy()) <= bound).all() and (np.abs(l2.astype(np.float64) - w2.numpy()) <= bound).all()
    assert 0.2 < (d1 > 0).mean() < 0.98                                          # both branches of the fallback
    ok, key, N = lm.shape_filter(np.ones(len(A), dtype=F32), L, A.reshape(-1, 4))
    Nw = torch.cat([torch.bmm(_t(A), _t(L[:, :, :2])), _t(L[:, :, 2:])], dim=2)
    bound = 2 * EPS * np.matmul(np.abs(A.astype(np.float64)), np.abs(L[:, :, :2].astype(np.float64))) + 1e-300
    _bmm_check("shape compose", N[:, :, :2], Nw.numpy()[:, :, :2], bound)
    m = lm.shape_filter_margins(L, A.reshape(-1, 4))
    clear = (m["corner"] > 1e-5) & (m["ratio6"] > 1e-3) & (m["ratio16"] > 1e-4)
    assert clear.mean() > 0.95
    ratio = torch.abs(w1 / (w2 + 1e-8))
    want = (((ratio < 6.0) & (ratio > (1.0 / 6.0))) & orc.inside_image(_t(N))).numpy()
    assert np.array_equal(ok, want)                                              # same composed frame in: the same decision, every row
    assert np.array_equal(ok[clear], (m["inside"] & m["ratio_ok"])[clear])      # and the float64 decision wherever it has a margin
    assert 0.1 < ok.mean() < 0.9
    c = lm.corners(N)
    cw = orc.frame_corners(_t(N)).numpy()
    bound = 2 * EPS * (np.abs(N[:, :, 0:1]) + np.abs(N[:, :, 1:2]) + np.abs(N[:, :, 2:3])).astype(np.float64)
    _bmm_check("frame corners", c, cw, np.broadcast_to(bound, c.shape))


def test_iterate_and_rotation_compose():
    rng = np.random.RandomState(2)
    n = 1000
    A, B, L = _rand_A(rng, n), _rand_A(rng, n), _rand_lafs(rng, n)
    base0, out0 = lm.shape_iterate(None, B.reshape(-1, 4), L, 0)
    assert np.array_equal(base0, B.reshape(-1, 4))
    base1, out1 = lm.shape_iterate(A.reshape(-1, 4), B.reshape(-1, 4), L, 1)
    wb = torch.bmm(_t(A), _t(B)).numpy()
    f64 = lambda x: np.abs(x.astype(np.float64))
    _bmm_check("iterate: base = A * base", base1.reshape(-1, 2, 2), wb, 2 * EPS * np.matmul(f64(A), f64(B)))
    wo = torch.bmm(_t(base1.reshape(-1, 2, 2)), _t(L[:, :, :2])).numpy()
    _bmm_check("iterate: base * LAF", out1[:, :, :2], wo, 2 * EPS * np.matmul(f64(base1.reshape(-1, 2, 2)), f64(L[:, :, :2])))
    assert np.array_equal(out1[:, :, 2], L[:, :, 2]) and np.array_equal(out0[:, :, 2], L[:, :, 2])
    ang = rng.uniform(-np.pi, np.pi, n).astype(F32)
    R = orc.angles_to_rotation(_t(ang)).numpy()
    got = lm.apply_rotation(L, R.reshape(-1, 4))
    wr = torch.bmm(_t(L[:, :, :2]), _t(R)).numpy()
    _bmm_check("apply rotation", got[:, :, :2], wr, 2 * EPS * np.matmul(f64(L[:, :, :2]), f64(R)))
    assert np.array_equal(got[:, :, 2], L[:, :, 2])


@pytest.mark.parametrize("wh", [(80, 64), (64, 80), (641, 481)])
def test_scale_lafs_is_the_oracles(wh):
    w, h = wh
    rng = np.random.RandomState(3)
    L = _rand_lafs(rng, 500)
    px = lm.scale_lafs(L, w, h, False)
    assert np.array_equal(px, orc.denormalize_lafs(_t(L), w, h).numpy())
    assert np.array_equal(lm.scale_lafs(px, w, h, True), orc.normalize_lafs(_t(px), w, h).numpy())
    c = lm.scale_consts(w, h, True)
    assert np.array_equal(np.array([[c[0], c[0], c[1]], [c[0], c[0], c[2]]], dtype=F32), orc.laf_scale_coef(w, h, inverse=True).numpy()[0])


def test_level_argmin_rule():
    """First minimum under strict `<`; equal sigmas resolve to the lower index; a NaN frame stays at level 0."""
    sig = np.array([1.6, 2.0, 2.5, 3.2, 4.0, 3.2, 4.0, 5.0, 6.4, 8.0])
    L = np.zeros((6, 2, 3), dtype=F32)
    for k, s in enumerate((3.2, 4.0, 1.0, 100.0, 2.25)):
        L[k, 0, 0] = L[k, 1, 1] = F32(s)                                         # ps = 1: the scale is the sigma itself
    L[5] = np.nan
    best, d = lm.level_argmin(L, 1, sig)
    assert best.tolist() == [3, 4, 0, 9, 1, 0]                                   # 2.25 is equally far from 2.0 and 2.5: the first wins
    ok = ~np.isnan(d).any(axis=1)
    assert np.array_equal(best[ok], np.argmin(d[ok], axis=1))
    mg = lm.level_margin(L[:5], 1, sig)
    assert mg[0] > 0.5 and mg[1] > 0.5                                           # on a doubled sigma the gap is to the NEXT value, not 0
    ids, norm = lm.level_select(L[:5], 1, sig, 5, 80, 64)
    assert ids.tolist()[:2] == [[0, 3, 0], [0, 4, 0]] and norm.dtype == F32


def test_reproject_lafs_against_the_oracle(golden_dir):
    import os
    H = np.load(os.path.join(golden_dir, "match_graf16_n500.npz"))["H"].astype(F32)
    rng = np.random.RandomState(5)
    n = 2000
    L = np.empty((n, 2, 3), dtype=F32)
    L[:, :, :2] = rng.normal(0.0, 15.0, (n, 2, 2))
    L[:, 0, 2], L[:, 1, 2] = rng.uniform(0, 800, n), rng.uniform(0, 640, n)
    for name, Hm in (("graf 1-6", H), ("identity", np.eye(3, dtype=F32))):
        got = lm.reproject_lafs(L, Hm)
        want = orc.reproject_lafs(_t(L), _t(Hm)).numpy()
        As = orc.lin_h(_t(Hm), _t(L[:, 0, 2]), _t(L[:, 1, 2])).numpy()
        f64 = lambda x: np.abs(x.astype(np.float64))
        _bmm_check("reproject " + name + ": linH * LAF", got[:, :, :2], want[:, :, :2], 2 * EPS * np.matmul(f64(As), f64(L[:, :, :2])) + 1e-300)
        x, y, h = L[:, 0, 2].astype(np.float64), L[:, 1, 2].astype(np.float64), Hm.astype(np.float64)
        Z = np.abs(h[2, 0] * x + h[2, 1] * y + h[2, 2])
        mag = np.stack([(abs(h[0, 0]) * x + abs(h[0, 1]) * y + abs(h[0, 2])), (abs(h[1, 0]) * x + abs(h[1, 1]) * y + abs(h[1, 2]))], axis=1) / Z[:, None]
        zmag = (abs(h[2, 0]) * x + abs(h[2, 1]) * y + abs(h[2, 2])) / Z
        _bmm_check("reproject " + name + ": centre", got[:, :, 2], want[:, :, 2], 4 * EPS * mag * (1.0 + zmag[:, None]))
    assert np.array_equal(lm.reproject_lafs(L, np.eye(3, dtype=F32)), L)       # the identity reprojects every frame onto itself, bit for bit


def test_centre_distances_against_the_oracle():
    rng = np.random.RandomState(6)
    q, r = np.zeros((300, 2, 3), dtype=F32), np.zeros((200, 2, 3), dtype=F32)
    q[:, :, 2], r[:, :, 2] = rng.uniform(700, 900, (300, 2)), rng.uniform(700, 900, (200, 2))
    r[50] = r[10]                                                              # an exact duplicate: the first index wins
    q[7, :, 2] = r[10, :, 2]
    d = lm.centre_distances(q, r)
    want = orc.distance_matrix_vector_reproj(_t(r[:, :, 2]), _t(q[:, :, 2])).numpy()
    assert want.shape == d.shape == (300, 200)
    sq = (q[:, :, 2].astype(np.float64) ** 2).sum(axis=1)[:, None] + (r[:, :, 2].astype(np.float64) ** 2).sum(axis=1)[None, :]
    # compared on the radicand: the root of a cancelled difference amplifies one ulp of the dot product without bound
    _bmm_check("centre distance radicand", d.astype(np.float64) ** 2, want.astype(np.float64) ** 2, 8 * EPS * sq)
    md, idx = lm.centre_nn(q, r)
    assert idx[7] == 10 and np.array_equal(md, d.min(axis=1)) and idx.dtype == np.int32
    true = np.sqrt(((q[:, None, :, 2].astype(np.float64) - r[None, :, :, 2]) ** 2).sum(axis=2))
    print("fp32 expansion at ~800 px: up to %.3g px from the true distance" % np.abs(d - true).max())
    assert np.abs(d - true).max() > 1e-3                                         # the cancellation the kernel must reproduce, not avoid


def test_ellipse_reference_error():
    frames, kind = lm.ellipse_frames()
    e_ref, got, want = lm.ellipse_reference_error(frames, kind)
    print("lafs_to_ellipses_t fp32 vs float64 restatement, relative to the row's largest coefficient: %s" % e_ref)
    record_parity("LAFs2ellT: the reference's own fp32 error (host)", **{"e_ref_" + k: v for k, v in e_ref.items()})
    assert 0.0 < e_ref["aniso"] < 1e-4 and 0.0 <= e_ref["iso"] < 1e-4, e_ref
    assert np.array_equal(got[:, :2], frames[:, :, 2]) and np.array_equal(want[:, :2].astype(F32), frames[:, :, 2])
    fin = np.isfinite(want)
    assert fin[(kind == "aniso") | (kind == "iso")].all()
    assert not fin[kind == "negdet"][:, 2:].any() and not fin[kind == "zero"][:, 2:].all(axis=1).any()
    assert np.array_equal(np.isfinite(got), fin)                                # the fp32 oracle has the restatement's non-finite pattern
    iso = frames[kind == "iso"]
    s2 = iso[:, 0, 0].astype(np.float64) ** 2
    assert np.allclose(want[kind == "iso"][:, 2], 1.0 / s2, rtol=1e-5) and np.allclose(want[kind == "iso"][:, 4], 1.0 / s2, rtol=1e-5)


def test_shape_filter_fixture_conditions():
    """The rows tests/test_gpu_laf_ops.py feeds the shape filter: no ambiguous row, every criterion decides both ways."""
    rows = lm.shape_rows()
    fig = lm.shape_rows_conditions(*rows)
    print("shape-filter fixture: %s" % fig)
    record_parity("shape-filter fixture margins (host)", **fig)
    grp = rows[4]
    for n in (255, 256, 257):
        assert {"ratio", "d1", "corner", "random"} <= set(grp[:n].tolist())
    assert 0.3 < fig["good"] / fig["rows"] < 0.7
    l1, l2, _ = lm.eig2x2(rows[3])
    assert int((np.abs(l1 / (l2 + F32(1e-8))) == F32(6.0))[:255].sum()) >= 2      # rows that tell `ratio < 6` from `<=`, inside every large count


@pytest.mark.parametrize("ps", [32, 19])
def test_level_fixture_conditions(ps):
    """The level table of a 64 x 80 context with three levels: equal sigmas in neighbouring octaves, and frames with a margin."""
    from _fp32_chain import pyramid_plan
    step = 2 ** (1.0 / 3.0)
    n_oct = len(pyramid_plan(64, 80, 3, 1.6, 5)[1])
    sig = []
    for o in range(n_oct):                                                     # HandCraftedModules.py:39-49 / LAF.py:459
        cur = 1.6
        for l in range(5):
            sig.append(cur * 2.0 ** o)
            cur *= step
    sig = np.array(sig)
    assert n_oct == 3 and sig[4] == sig[6] and sig[9] == sig[11] and sig[3] != sig[5]
    F, T, K = lm.level_frames(sig, ps)
    best, d = lm.level_argmin(F, ps, sig)
    mg = lm.level_margin(F, ps, sig)
    keep = K != "nan"
    print("level fixture, ps %d: smallest gap between distinct sigma values %.3g; levels chosen %s" % (ps, mg[keep].min(), sorted(set(best.tolist()))))
    assert mg[keep].min() > 1e-6
    assert 6 not in best and 11 not in best and (best == 4).sum() > 5 and (best == 9).sum() > 5     # equal sigmas: the lower (octave, level)
    assert best[K == "nan"].tolist() == [0]
    assert set(K[:255].tolist()) == {"on", "near", "out", "mid", "nan"}
