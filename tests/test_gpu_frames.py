"""GPU tests of the caller-supplied-frames path: affnet_load_frames / affnet_describe_frames / affnet_ellipses_to_lafs and their host
mirror (enqueue_frames, describe_frames, getAffineShape, getOrientation, LAF.ells2LAFsT, examples/hesaffnet/describe_keypoints.py).
240x320 synthetic image, seed 1; the extractor's constructor defaults (mrSize 3, border 16)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _frames as fr
import affnet_oracle as orc
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARITH = ["fp32", "fp32_split3", "fp32_split2h"]
OVF_COUNT, OVF_NONFINITE = 16, 32            # include/affnet_hip.h, affnet_read_counts


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return affnet_amd


@pytest.fixture(scope="module")
def nets(amd, weights):
    A = amd.AffNetFast(PS=32); A.load_state_dict(weights["AffNet"]); A = A.to(DEV)
    O = amd.OriNetFast(PS=32); O.load_state_dict(weights["OriNet"]); O = O.to(DEV)
    Hn = amd.HardNet(); Hn.load_state_dict(weights["HardNet"]); Hn = Hn.to(DEV)
    return A, O, Hn


@pytest.fixture(scope="module")
def image_a():
    return orc.synthetic_image(fr.H, fr.W, 1).to(DEV)


def _extractor(amd, nets, n=300, iters=1, arith="fp32", lazy=-1):
    A, O, _ = nets
    det = amd.ScaleSpaceAffinePatchExtractor(num_features=n, num_Baum_iters=iters, AffNet=A, OriNet=O, arith=arith).to(DEV)
    det.lazy_shape_rows = lazy
    return det


def _st():
    from affnet_amd import engine
    return engine.stream_of(torch.device(DEV))


def _detected_list(ctx):
    from affnet_amd._lib import lib, check, ptr
    P, B = ctx.cap_pre, ctx.batch
    out = (torch.empty(B, P, device=DEV), torch.empty(B, P, 2, 3, device=DEV), torch.empty(B, P, 3, dtype=torch.int32, device=DEV),
           torch.zeros(B, dtype=torch.int32, device=DEV))
    check(lib.affnet_detected_list(ctx.handle, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), _st()), ctx.handle, "affnet_detected_list")
    torch.cuda.synchronize()
    return out


def _load_frames(ctx, lafs, normalised, resp, ids, count, n_max, ps):
    from affnet_amd._lib import lib, ptr
    return lib.affnet_load_frames(ctx.handle, ptr(lafs), int(normalised), ptr(resp), ptr(ids), ptr(count), int(n_max), int(ps), _st())


def _laf_bar(Lw, ori_norm):
    """tests/test_gpu_parity.py::_laf_bar restated: per-row LAF tolerance max(1e-3 px, S (1e-5 + 4e-5 / |o|)), S = sqrt|det A| px, |o| = the
    length of OriNet's vector before atan2 (two fp32 summation orders of the CNNs differ by ~1e-5 relative at AffNet's output and by that
    over |o| in the angle)."""
    S = np.sqrt(np.abs(Lw[:, 0, 0] * Lw[:, 1, 1] - Lw[:, 0, 1] * Lw[:, 1, 0]))
    return np.maximum(1e-3, S * (1e-5 + 4e-5 / np.maximum(ori_norm, 1e-12)))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("lazy", [-1, 0])
def test_detection_list_round_trip_is_bit_identical(amd, nets, image_a, arith, lazy):
    """The detector's own list, saved, overwritten by another image's detections and handed back through affnet_load_frames, describes to
    exactly the rows of the fused call: the ingest leaves the context as a detector half does."""
    from affnet_amd._lib import lib, check, ptr
    Hn = nets[2]
    det = _extractor(amd, nets, arith=arith, lazy=lazy)
    first = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in det.enqueue(image_a, do_ori=True, desc=Hn).items()}
    ctx = det._ctx
    resp, lafs, ids, cnt = _detected_list(ctx)
    assert int(cnt[0]) == 450
    det.enqueue(orc.synthetic_image(fr.H, fr.W, 2).to(DEV), do_ori=True, desc=Hn)          # every internal list and counter overwritten
    torch.cuda.synchronize()
    assert not torch.equal(_detected_list(ctx)[1], lafs)
    F = ctx.cap_final
    out = {"LAFs": torch.empty(F, 2, 3, device=DEV), "responses": torch.empty(F, device=DEV), "ids": torch.empty(F, 3, dtype=torch.int32, device=DEV),
           "descriptors": torch.empty(F, 128, device=DEV), "count": torch.zeros(1, dtype=torch.int32, device=DEV)}
    img = image_a.contiguous().float()
    check(lib.affnet_pyramid_build(ctx.handle, ptr(img), _st()), ctx.handle, "affnet_pyramid_build")
    assert _load_frames(ctx, lafs, 1, resp, ids, cnt, ctx.cap_pre, 32) == 0
    nn_ = det._nets(torch.device(DEV), True, Hn)
    check(lib.affnet_describe_detected(ctx.handle, C.byref(nn_), 1, ptr(out["LAFs"]), ptr(out["responses"]), ptr(out["ids"]), ptr(out["descriptors"]),
                                       ptr(out["count"]), _st()), ctx.handle, "affnet_describe_detected")
    counts = ctx.read_counts()
    assert counts[0] == 450 and counts[1] == int(first["count"][0]) > 0 and counts[2] == 0
    for k in out:
        assert torch.equal(out[k], first[k]), k


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [32, 19])
def test_level_rule_equals_level_select(amd, nets, image_a, weights, ps):
    from affnet_amd._lib import lib, check, ptr
    frames = fr.foreign_frames(weights)[2].to(DEV)                          # 450 pixel frames on several octaves and levels
    n = frames.size(0)
    det = _extractor(amd, nets, n=400)                                       # capacity 600 > 450: rows past n_max must come out zero
    det.enqueue(image_a)
    ctx = det._ctx
    assert ctx.cap_pre == 600
    assert _load_frames(ctx, frames, 0, None, None, None, n, ps) == 0
    resp, lafs, ids, cnt = [t[0] for t in _detected_list(ctx)]
    ids_w = torch.empty(n, 3, dtype=torch.int32, device=DEV)
    norm_w = torch.empty(n, 2, 3, device=DEV)
    check(lib.affnet_level_select(ctx.handle, ptr(frames), None, n, ps, ptr(ids_w), ptr(norm_w), _st()), ctx.handle, "affnet_level_select")
    torch.cuda.synchronize()
    assert int(cnt) == n
    assert torch.equal(ids[:n, :2], ids_w[:, :2]) and torch.equal(lafs[:n], norm_w)
    assert torch.equal(ids[:n, 2], torch.arange(n, dtype=torch.int32, device=DEV))
    assert torch.equal(resp[:n], torch.arange(n, 0, -1, device=DEV).float())
    assert not resp[n:].any() and not lafs[n:].any() and not ids[n:].any()
    assert len(set(map(tuple, ids[:n, :2].cpu().tolist()))) >= 5
    # normalised input: same levels (the scale is taken from the frame denormalised as affnet_scale_lafs does it), frames copied through
    from affnet_amd.LAF import denormalizeLAFs
    assert _load_frames(ctx, norm_w, 1, None, None, None, n, ps) == 0
    _, lafs2, ids2, _ = [t[0] for t in _detected_list(ctx)]
    px, scratch = denormalizeLAFs(norm_w, fr.W, fr.H), torch.empty_like(norm_w)
    check(lib.affnet_level_select(ctx.handle, ptr(px), None, n, ps, ptr(ids_w), ptr(scratch), _st()), ctx.handle, "affnet_level_select")
    torch.cuda.synchronize()
    assert torch.equal(lafs2[:n], norm_w) and torch.equal(ids2[:n, :2], ids_w[:, :2])


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", [450, 200])
def test_foreign_frames_against_the_oracle(amd, nets, image_a, weights, n_out):
    """Frames the detector never produced (tests/_frames.py: permuted, sheared, rotated, rescaled candidates with unsorted responses) through
    ONE describe_frames call against the unchanged oracle stages.  n_out = 450: nothing to cut (nonzero branch); 200: top-k branch.
    Bars = the project's (tests/test_gpu_parity.py::_laf_bar): responses bit-equal, >= 99.5 % of the LAF rows within 1e-3 px, none outside
    5e-3 px, every row inside max(1e-3 px, S (1e-5 + 4e-5 / |o|)), descriptors within 1e-3."""
    o = fr.oracle_on_frames(weights, n_out)
    ratio_margin, corner_margin = fr.margins(o["stage"])
    assert ratio_margin > 1e-3 and corner_margin > 1e-4, "a borderline oracle decision: the same-set requirement below would not be fair"
    assert int(o["stage"]["good"].sum()) == 292
    _, _, frames, resp = fr.foreign_frames(weights)
    det = _extractor(amd, nets, n=n_out)
    r = det.describe_frames(image_a, frames.to(DEV), responses=resp.to(DEV), do_ori=True, desc=nets[2])
    rows = r["ids"][:, 2].cpu().numpy()
    assert len(rows) == len(o["rows"]) == min(292, n_out)
    assert np.array_equal(np.sort(rows), np.sort(o["rows"])), "not the same set of source rows"
    if n_out == 450:
        assert np.array_equal(rows, o["rows"])                                     # survivors in caller order
    pos = {int(v): k for k, v in enumerate(o["rows"])}
    wi = np.array([pos[int(v)] for v in rows])
    L, Lw = r["LAFs"].cpu().numpy().astype(np.float64), o["LAFs"][wi].astype(np.float64)
    assert np.array_equal(r["responses"].cpu().numpy(), o["resp"][wi])
    dl = np.abs(L - Lw).reshape(len(rows), -1).max(axis=1)
    nv = np.linalg.norm(o["ori_vec"].astype(np.float64), axis=1)[wi]
    bar = _laf_bar(Lw, nv)
    dd = np.abs(r["descriptors"].cpu().numpy() - o["desc"][wi]).max(axis=1)
    lv = set(map(tuple, np.stack([o["oct"], o["lev"]], 1).tolist()))
    record_parity("caller-supplied frames vs the oracle, 320x240, N = %d" % n_out, frames=450, rows=int(len(rows)), laf_max_px=float(dl.max()),
                  laf_rows_within_1e_3=float((dl < 1e-3).mean()), worst_over_bar=float((dl / bar).max()), desc_max=float(dd.max()),
                  orinet_norm_min=float(nv.min()), ratio_margin_log=ratio_margin, corner_margin=corner_margin, pyramid_levels_used=len(lv))
    print("n_out %d: laf max %.3g px, within 1e-3: %.4f, worst/bar %.3g, desc max %.3g" % (n_out, dl.max(), (dl < 1e-3).mean(), (dl / bar).max(), dd.max()))
    assert (dl < 1e-3).mean() >= 0.995 and dl.max() <= 5e-3
    assert (dl <= bar).all()
    assert dd.max() < 1e-3


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_sorted_and_unsorted_rows_give_the_same_output(amd, nets, image_a, weights):
    """N = 200 of 292 survivors: caller order (unsorted responses: general top-N, AffNet on every row) against the same rows pre-sorted by
    descending response (verified by the ingest: prefix selection, lazy second AffNet pass skipped)."""
    o = fr.oracle_on_frames(weights, 200)
    _, _, frames, resp = fr.foreign_frames(weights)
    order = torch.argsort(resp, descending=True, stable=True)
    # the lazy window: a few rows past the 200th survivor in response order (the oracle's decisions; their margins are asserted in test 3)
    need = int(np.searchsorted(np.cumsum(o["stage"]["good"].numpy()[order.numpy()]), 200)) + 1
    lazy = need + 8
    assert lazy < 450
    det = _extractor(amd, nets, n=200, lazy=lazy)
    Hn = nets[2]
    a = det.describe_frames(image_a, frames.to(DEV), responses=resp.to(DEV), do_ori=True, desc=Hn)
    a = {k: v.clone() for k, v in a.items()}
    ev_unsorted = int(det._fctx.counter_view(3)[0])
    b = det.describe_frames(image_a, frames[order].to(DEV), responses=resp[order].to(DEV), do_ori=True, desc=Hn)
    ev_sorted = int(det._fctx.counter_view(3)[0])
    assert a["LAFs"].shape[0] == b["LAFs"].shape[0] == 200
    assert torch.equal(order.to(DEV)[b["ids"][:, 2].long()].int(), a["ids"][:, 2])            # same source rows in the same output order
    for k in ("LAFs", "responses", "descriptors"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["ids"][:, :2], b["ids"][:, :2])
    assert ev_unsorted == 450 and ev_sorted == lazy, (ev_unsorted, ev_sorted, lazy)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_row_counts_and_ragged_batch(amd, nets, image_a, weights):
    """Counts around the 64-lane and 256-thread edges of the ingest and row loops, the capacity itself, and a ragged batch."""
    from affnet_amd import _lib
    Hn = nets[2]
    cap = 257
    frames = fr.foreign_frames(weights)[2][:cap].to(DEV)
    det = _extractor(amd, nets, n=300)                                       # budget >= n_max: no cut, survivors in caller order
    xb = orc.synthetic_image(fr.H, fr.W, 2).to(DEV)
    single = {}
    for img_name, img in (("a", image_a), ("b", xb)):
        for c in (0, 1, 63, 64, 65, 255, 256, 257):
            if img_name == "b" and c != 0:
                continue
            r = det.enqueue_frames(img, frames, counts=[c], do_ori=True, desc=Hn)
            ctx = det._fctx
            assert ctx.cap_pre == cap
            rc = _lib.lib.affnet_read_counts(ctx.handle, C.byref((C.c_int32 * 4)()), _st())
            assert rc == (_lib.ERR_EMPTY if c == 0 else _lib.OK), (c, rc)
            n = int(r["count"][0])
            assert n <= c
            for k in ("LAFs", "responses", "ids", "descriptors"):
                assert not r[k][n:].any(), (c, k)                                # rows >= count are zero in every output
            src = r["ids"][:n, 2]
            assert (src[1:] > src[:-1]).all() and (n == 0 or int(src[-1]) < c)       # d_resp == NULL keeps caller order
            single[(img_name, c)] = {k: r[k].clone() for k in ("LAFs", "responses", "ids", "descriptors", "count")}
    full = single[("a", 257)]
    assert int(full["count"][0]) > 100
    for c in (1, 63, 64, 65, 255, 256):                                          # a shorter list = the rows of the full list that come from rows < c
        n = int(single[("a", c)]["count"][0])
        keep = (full["ids"][:, 2] < c) & (torch.arange(cap, device=DEV) < int(full["count"][0]))
        assert int(keep.sum()) == n
        for k in ("LAFs", "ids", "descriptors"):
            assert torch.equal(single[("a", c)][k][:n], full[k][keep]), (c, k)
        # responses are n_max - i: the same whatever the count
        assert torch.equal(single[("a", c)]["responses"][:n], full["responses"][keep])
    xs = torch.cat([image_a, xb, image_a], 0)
    r = det.enqueue_frames(xs, frames.unsqueeze(0).expand(3, cap, 2, 3).contiguous(), counts=torch.tensor([65, 0, 257], dtype=torch.int32, device=DEV),
                           do_ori=True, desc=Hn)
    ctx = det._fctx
    assert _lib.lib.affnet_read_counts(ctx.handle, C.byref((C.c_int32 * 4)()), _st()) == _lib.OK        # one empty image is not an error
    for b, key in enumerate((("a", 65), ("b", 0), ("a", 257))):
        for k in ("LAFs", "responses", "ids", "descriptors"):
            assert torch.equal(r[k][b], single[key][k]), (b, k)
        assert int(r["count"][b]) == int(single[key]["count"][0])
    lst = det.describe_frames(xs, frames.unsqueeze(0).expand(3, cap, 2, 3).contiguous(), counts=[65, 0, 257], do_ori=True, desc=Hn)
    assert [d["LAFs"].shape[0] for d in lst] == [int(single[k]["count"][0]) for k in (("a", 65), ("b", 0), ("a", 257))]
    with pytest.raises(_lib.AffnetEmptyError):
        det.describe_frames(image_a, frames[:0], do_ori=True, desc=Hn)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_contained_by_the_ingest(amd, weights):
    """Ingest only - nothing runs on these lists: non-finite rows become zero rows and an error at the read-back, an oversized n_max is
    refused at the call, an oversized device count is clamped and flagged."""
    from affnet_amd import _lib, engine
    ctx = engine.Context(fr.H, fr.W, torch.device(DEV), 3, 1.6, fr.BORDER, fr.MR, 0.0, 64, 64)
    assert ctx.cap_pre == 64
    clean = fr.foreign_frames(weights)[2][:64].to(DEV)
    resp = torch.arange(64, 0, -1, device=DEV).float() * 0.5
    assert _load_frames(ctx, clean, 0, resp, None, None, 64, 32) == 0
    r0, l0, i0, c0 = [t[0].clone() for t in _detected_list(ctx)]
    counts = (C.c_int32 * 4)()
    assert _lib.lib.affnet_read_counts(ctx.handle, C.byref(counts), _st()) == _lib.OK and counts[0] == 64 and counts[2] == 0
    bad = clean.clone()
    bad[10, 1, 0] = float("nan")
    bad[20, 0, 2] = float("inf")
    assert _load_frames(ctx, bad, 0, resp, None, None, 64, 32) == 0
    r1, l1, i1, c1 = [t[0] for t in _detected_list(ctx)]
    ok = torch.ones(64, dtype=torch.bool, device=DEV)
    ok[[10, 20]] = False
    assert not l1[~ok].any() and not r1[~ok].any() and torch.isfinite(l1).all()
    assert torch.equal(l1[ok], l0[ok]) and torch.equal(r1[ok], r0[ok]) and torch.equal(i1[ok], i0[ok])      # neighbours bit-unchanged
    assert torch.equal(i1[:, 2], torch.arange(64, dtype=torch.int32, device=DEV)) and int(c1) == 64
    rc = _lib.lib.affnet_read_counts(ctx.handle, C.byref(counts), _st())
    msg = _lib.lib.affnet_last_error(ctx.handle).decode()
    assert rc == _lib.ERR_INVALID and "not finite" in msg and (counts[2] & OVF_NONFINITE), (rc, msg)
    assert int(ctx.counter_view(0)[0]) & OVF_NONFINITE
    # a non-finite response alone does it too
    rb = resp.clone()
    rb[5] = float("-inf")
    assert _load_frames(ctx, clean, 0, rb, None, None, 64, 32) == 0
    r2, l2, _, _ = [t[0] for t in _detected_list(ctx)]
    assert float(r2[5]) == 0 and not l2[5].any() and _lib.lib.affnet_read_counts(ctx.handle, C.byref(counts), _st()) == _lib.ERR_INVALID
    # n_max above the capacity: refused at the call, nothing enqueued
    big = torch.zeros(65, 2, 3, device=DEV)
    assert _load_frames(ctx, big, 0, None, None, None, 65, 32) == _lib.ERR_INVALID
    assert "n_max" in _lib.lib.affnet_last_error(ctx.handle).decode()
    # a device count above n_max: clamped, flagged
    c_big, c_neg = torch.tensor([100], dtype=torch.int32, device=DEV), torch.tensor([-3], dtype=torch.int32, device=DEV)
    assert _load_frames(ctx, clean, 0, resp, None, c_big, 64, 32) == 0
    r3, l3, _, c3 = [t[0] for t in _detected_list(ctx)]
    assert int(c3) == 64 and torch.equal(l3, l0) and int(ctx.counter_view(0)[0]) == OVF_COUNT and int(ctx.counter_view(1)[0]) == 64
    assert _lib.lib.affnet_read_counts(ctx.handle, C.byref(counts), _st()) == _lib.ERR_CAPACITY and counts[2] == OVF_COUNT
    # and a clean call afterwards clears the flags
    assert _load_frames(ctx, clean, 0, resp, None, c_neg, 64, 32) == 0
    assert _lib.lib.affnet_read_counts(ctx.handle, C.byref(counts), _st()) == _lib.ERR_EMPTY and counts[2] == 0


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_get_affine_shape_and_orientation_equal_the_fused_path(amd, nets, image_a):
    """The reference's two public methods on the saved detector list = forward(do_ori=True), bit for bit (the staged and
    the fused path agree bit for bit)."""
    from affnet_amd.LAF import denormalizeLAFs
    det = _extractor(amd, nets)
    z = torch.zeros(1, 2, 3, device=DEV)
    with pytest.raises(RuntimeError):
        det.getAffineShape(torch.zeros(1, device=DEV), z, torch.zeros(1), torch.zeros(1), 300)
    with pytest.raises(RuntimeError):
        det.getOrientation(z, torch.zeros(1), torch.zeros(1))
    L, r = det(image_a, do_ori=True)
    L, r = L.clone(), r.clone()
    resp, lafs, ids, cnt = [t[0] for t in _detected_list(det._ctx)]
    n = int(cnt)
    r2, l2, o2, v2 = det.getAffineShape(resp[:n], lafs[:n], ids[:n, 0], ids[:n, 1], 300)
    assert l2.shape[0] == 300 and torch.equal(r2, r)
    assert torch.equal(o2.int(), ids[det.last_ids[:, 2].long(), 0]) and torch.equal(v2.int(), ids[det.last_ids[:, 2].long(), 1])
    l3 = det.getOrientation(l2, o2, v2)
    assert torch.equal(denormalizeLAFs(l3, fr.W, fr.H), L)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_ells2lafs_on_the_device_against_the_golden(amd):
    from affnet_amd.LAF import LAFs2ellT, ells2LAFsT
    ells, lafs, bar, bar_rt, m = fr.golden_ells()
    e = torch.from_numpy(ells).to(DEV)
    got = ells2LAFsT(e)
    err = fr.shape_err(got.cpu().numpy(), lafs)
    assert torch.equal(got[:, :, 2], e[:, :2])                                   # centres bit for bit
    back = LAFs2ellT(got)
    rt = fr.ell_rel_err(back.cpu().numpy(), ells)
    record_parity("ells2LAFsT on the device vs the reference's golden output (603 ellipses)", worst_over_frame_scale=float(err.max()), bar=bar,
                  round_trip_worst_relative=float(rt.max()), round_trip_bar=bar_rt, **m)
    print("ells2LAFsT: worst %.3g (bar %.3g); round trip %.3g (bar %.3g); reference's own %s" % (err.max(), bar, rt.max(), bar_rt, m))
    assert err.max() <= bar
    assert torch.equal(back[:, :2], e[:, :2]) and rt.max() <= bar_rt
    # rows >= count are zero
    from affnet_amd import engine
    from affnet_amd._lib import lib, check, ptr
    out = torch.full((603, 2, 3), 7.0, device=DEV)
    ctx = engine.utility_ctx(torch.device(DEV))
    cnt = torch.tensor([300], dtype=torch.int32, device=DEV)
    check(lib.affnet_ellipses_to_lafs(ctx, ptr(e), ptr(cnt), 603, ptr(out), _st()), ctx, "affnet_ellipses_to_lafs")
    torch.cuda.synchronize()
    assert torch.equal(out[:300], got[:300]) and not out[300:].any()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_describe_keypoints_cli(amd, nets, image_a, tmp_path):
    """Image A's frames written with the Oxford writer and described by examples/hesaffnet/describe_keypoints.py."""
    from PIL import Image
    from affnet_amd.LAF import LAFs2ellT
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    u8 = image_a[0, 0].round().clamp(0, 255).byte()
    Image.fromarray(u8.cpu().numpy()).save(tmp_path / "a.png")
    det = _extractor(amd, nets)
    L, _ = det(u8.float()[None, None], do_ori=False)
    ell_in = LAFs2ellT(L).cpu().numpy()
    with open(tmp_path / "in.txt", "w") as f:
        f.write("1.0\n%d\n" % len(ell_in))
        np.savetxt(f, ell_in, delimiter=" ", fmt="%10.10f")
    out = tmp_path / "out.txt"
    subprocess.check_call([sys.executable, os.path.join(root, "examples/hesaffnet/describe_keypoints.py"), str(tmp_path / "a.png"), str(tmp_path / "in.txt"),
                           str(out), "--no-shape"])
    lines = open(out).read().split("\n")
    ell = np.loadtxt(out, skiprows=2, ndmin=2)
    desc, rows = np.load(str(out) + ".desc.npy"), np.load(str(out) + ".rows.npy")
    assert lines[0].strip() == "1.0" and int(lines[1]) == len(ell) == len(ell_in) == 300
    assert np.array_equal(rows, np.arange(300))
    assert np.array_equal(ell[:, :2].astype(np.float32), np.loadtxt(tmp_path / "in.txt", skiprows=2)[:, :2].astype(np.float32))     # centres exact
    assert desc.shape == (300, 128) and np.allclose(np.linalg.norm(desc, axis=1), 1.0, atol=1e-4)
    # with the shape stage: the survivors of the shape filter, each at the centre of the input row it names
    subprocess.check_call([sys.executable, os.path.join(root, "examples/hesaffnet/describe_keypoints.py"), str(tmp_path / "a.png"), str(tmp_path / "in.txt"),
                           str(out), "--desc", "sift"])
    ell = np.loadtxt(out, skiprows=2, ndmin=2)
    desc, rows = np.load(str(out) + ".desc.npy"), np.load(str(out) + ".rows.npy")
    assert int(open(out).read().split("\n")[1]) == len(ell) == len(rows) and 0 < len(rows) <= 300 and desc.shape == (len(rows), 128)
    assert np.array_equal(ell[:, :2].astype(np.float32), np.loadtxt(tmp_path / "in.txt", skiprows=2)[rows, :2].astype(np.float32))
    record_parity("describe_keypoints.py: 300 regions of hesaffnet's own output described again", rows_kept_by_the_shape_filter=int(len(rows)))
