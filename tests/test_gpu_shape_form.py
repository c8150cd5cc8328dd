"""The two forms of the fused AffNet shape pass (affnet_set_shape_form, the extractor's `shape_form`): 0 = the direct trunk on every candidate, 1 = the
trunk with Winograd conv1 / conv3 on every candidate, the margin rule (affnet_amd/csrc/shape_filter.h: aff_shape_margin_flag) and the direct trunk on the
flagged candidates.  Form 1 must take every decision as form 0 does - counts, ids and responses bit-equal - and may differ from it only by the Winograd
rounding of A on unflagged candidates (at most delta = 4e-6).  Three synthetic 320x240 images (seeds 0, 1, 2), 300 features = 450 candidates each, the
benchmark's extractor settings; read-back of A and the flags through libaffnet_hip_probes.so (affnet_probe_shape_offsets)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _shape_margin as sm
import affnet_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = (0, 1, 2)
KEYS = ("LAFs", "responses", "ids", "descriptors", "count")


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
def images():
    return torch.cat([orc.synthetic_image(sm.H, sm.W, s) for s in SEEDS]).to(DEV)


@pytest.fixture(scope="module")
def probes():
    from affnet_amd import _lib
    assert os.path.isfile(_lib.PROBES_LIB_PATH), "libaffnet_hip_probes.so is missing (AFFNET_PROBES=1 bash affnet_amd/csrc/build.sh)"
    pl = C.CDLL(_lib.PROBES_LIB_PATH)
    pl.affnet_probe_shape_offsets.restype, pl.affnet_probe_shape_offsets.argtypes = _lib.PROBE_SYMBOLS["affnet_probe_shape_offsets"]
    return pl


def _extractor(amd, nets, form, lazy=-1):
    det = amd.ScaleSpaceAffinePatchExtractor(mrSize=sm.MR_SIZE, num_features=sm.N_FEATURES, border=sm.BORDER, num_Baum_iters=1, AffNet=nets[0],
                                             OriNet=nets[1]).to(DEV)
    det.shape_form, det.lazy_shape_rows = form, lazy
    return det


def _full(det, x, Hn):
    r = det.enqueue(x, do_ori=True, desc=Hn)
    torch.cuda.synchronize()
    assert det._ctx.read_counts()[2] == 0
    return {k: r[k].clone() for k in KEYS}


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _offsets(probes, ctx):
    out = (C.c_int64 * 3)()
    assert probes.affnet_probe_shape_offsets(ctx.handle, C.byref(out)) == 0
    return list(out)


def _shape_rows(probes, det, x):
    """The shape pass alone (no orientation, no descriptors: they reuse the scratch the flags live in): A and flags of every candidate, the candidates'
    frames, and the per-image counters (candidates evaluated, candidates recomputed)"""
    r = det.enqueue(x, do_ori=False, desc=None)
    torch.cuda.synchronize()
    ctx = det._ctx
    B, P = ctx.batch, ctx.cap_pre
    oA, oF, oL = _offsets(probes, ctx)
    A = ctx.workspace.view(torch.float32)[oA:oA + B * P * 4].view(B, P, 4).cpu().numpy().copy()
    flags = ctx.workspace.view(torch.int32)[oF:oF + B * P].view(B, P).cpu().numpy().copy()
    lafs = ctx.workspace.view(torch.float32)[oL:oL + B * P * 6].view(B, P, 6).cpu().numpy().copy()
    return {"A": A, "flags": flags, "lafs": lafs, "evaluated": ctx.counter_view(3).cpu().numpy().copy(), "recomputed": ctx.counter_view(4).cpu().numpy().copy(),
            "out": {k: r[k].clone() for k in ("LAFs", "responses", "ids", "count")}}


@pytest.mark.parametrize("lazy", [-1, 100])
def test_form1_decides_as_form0(amd, nets, images, lazy):
    """lazy = 100: the first pass cannot reach 300 survivors, so the second pass certainly runs"""
    want = _full(_extractor(amd, nets, 0, lazy), images, nets[2])
    got = _full(_extractor(amd, nets, 1, lazy), images, nets[2])
    assert int(want["count"].min()) > 0
    assert _bits_equal(got["count"], want["count"])
    dl = dd = 0.0
    for b, n in enumerate(want["count"].tolist()):                # rows past the count are not part of the result
        for k in ("ids", "responses"):
            assert _bits_equal(got[k][b, :n], want[k][b, :n]), "image %d: %s" % (b, k)
        dl = max(dl, float((got["LAFs"][b, :n] - want["LAFs"][b, :n]).abs().max()))
        dd = max(dd, float((got["descriptors"][b, :n] - want["descriptors"][b, :n]).abs().max()))
    print("lazy %d: rows %s; form 1 - form 0: LAFs max %.3g px, descriptors max %.3g" % (lazy, want["count"].tolist(), dl, dd))
    assert dl <= 1e-3 and dd <= 1e-3


@pytest.mark.parametrize("lazy", [-1, 100])
def test_flagged_rows_carry_the_direct_bits(amd, nets, images, probes, lazy):
    r0 = _shape_rows(probes, _extractor(amd, nets, 0, lazy), images)
    r1 = _shape_rows(probes, _extractor(amd, nets, 1, lazy), images)
    assert _bits_equal(r1["out"]["count"], r0["out"]["count"])
    for b, n in enumerate(r0["out"]["count"].tolist()):
        for k in ("ids", "responses"):
            assert _bits_equal(r1["out"][k][b, :n], r0["out"][k][b, :n]), "image %d: %s" % (b, k)
    assert (r0["evaluated"] == r1["evaluated"]).all() and (r0["recomputed"] == 0).all()
    if lazy == 100:
        assert (r1["evaluated"] > 100).all(), "the second pass did not run"
    for b in range(len(SEEDS)):
        n = int(r1["evaluated"][b])
        flag = r1["flags"][b, :n] != 0
        A0, A1 = r0["A"][b, :n], r1["A"][b, :n]
        dA = np.abs(A1.astype(np.float64) - A0)
        print("lazy %d image %d: %d evaluated, %d flagged (counter %d, %.2f %%), |dA| max on unflagged rows %.3g"
              % (lazy, b, n, int(flag.sum()), int(r1["recomputed"][b]), 100.0 * flag.mean(), float(dA[~flag].max())))
        assert set(np.unique(r1["flags"][b, :n])) <= {0, 1}
        assert (A1[flag].view(np.uint32) == A0[flag].view(np.uint32)).all(), "a flagged row does not carry the direct kernel's A"
        assert float(dA[~flag].max()) <= sm.DELTA
        assert int(flag.sum()) == int(r1["recomputed"][b])
        assert flag.mean() <= sm.FLAGGED_SHARE_CAP
        # the device's rule is the mirror's: an unflagged row still holds the Winograd A the rule saw
        assert not sm.margin_flag(A1[~flag], r1["lafs"][b, :n][~flag]).any()


def test_runs_batches_and_graph_replay_agree(amd, nets, images):
    Hn = nets[2]
    det = _extractor(amd, nets, 1)
    a = _full(det, images, Hn)
    b = _full(det, images, Hn)
    assert _bits_equal(a["count"], b["count"])
    for i, n in enumerate(a["count"].tolist()):
        for k in ("LAFs", "responses", "ids", "descriptors"):
            assert _bits_equal(a[k][i, :n], b[k][i, :n]), "second run, image %d: %s" % (i, k)
    one = _extractor(amd, nets, 1)
    for i in range(len(SEEDS)):
        s = _full(one, images[i:i + 1], Hn)
        n = int(a["count"][i])
        assert int(s["count"][0]) == n
        for k in ("LAFs", "responses", "ids", "descriptors"):
            assert _bits_equal(s[k][:n], a[k][i, :n]), "B = 1 call of image %d: %s" % (i, k)
    cap = _extractor(amd, nets, 1).capture(images[:1], do_ori=True, desc=Hn)
    for i in (1, 0):
        g = cap.run(images[i:i + 1])
        n = int(a["count"][i])
        for k in ("LAFs", "responses", "ids", "descriptors"):
            assert _bits_equal(g[k], a[k][i, :n]), "graph replay of image %d: %s" % (i, k)


def test_constant_patch_and_nan_frame_give_form0s_rows(amd, nets, images, probes):
    """A candidate whose frame has a zero 2x2 part (all 1024 samples at one point: a constant patch) and one with a NaN frame, planted in the detector's list
    between the two halves of the call: form 1 returns form 0's rows (ids and responses bit for bit), and the NaN row carries the direct kernel's A."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, check, ptr
    x = images[:1]
    Hn = nets[2]
    out = {}
    for form in (0, 1):
        det = _extractor(amd, nets, form)
        ctx = det._context(x)
        st = engine.stream_of(torch.device(DEV))
        img = x.contiguous().float()
        check(lib.affnet_detect_image(ctx.handle, ptr(img), st), ctx.handle, "affnet_detect_image")
        torch.cuda.synchronize()
        oA, oF, oL = _offsets(probes, ctx)
        lafs = ctx.workspace.view(torch.float32)[oL:oL + ctx.cap_pre * 6].view(ctx.cap_pre, 6)
        lafs[3] = torch.tensor([0.0, 0.0, 0.4, 0.0, 0.0, 0.6], device=DEV)
        lafs[7, 1] = float("nan")
        F = ctx.cap_final
        o = {"LAFs": torch.empty(F, 2, 3, device=DEV), "responses": torch.empty(F, device=DEV), "ids": torch.empty(F, 3, dtype=torch.int32, device=DEV),
             "descriptors": torch.empty(F, 128, device=DEV), "count": torch.zeros(1, dtype=torch.int32, device=DEV)}
        nn_ = det._nets(torch.device(DEV), True, Hn)
        check(lib.affnet_describe_detected(ctx.handle, C.byref(nn_), 1, ptr(o["LAFs"]), ptr(o["responses"]), ptr(o["ids"]), ptr(o["descriptors"]),
                                           ptr(o["count"]), st), ctx.handle, "affnet_describe_detected")
        torch.cuda.synchronize()
        A = ctx.workspace.view(torch.float32)[oA:oA + ctx.cap_pre * 4].view(ctx.cap_pre, 4).cpu().numpy().copy()
        out[form] = (o, A, int(ctx.counter_view(4)[0]))
    (o0, A0, _), (o1, A1, recomputed) = out[0], out[1]
    n = int(o0["count"][0])
    assert n > 0 and int(o1["count"][0]) == n
    for k in ("responses", "ids"):
        assert _bits_equal(o1[k][:n], o0[k][:n]), k
    # the NaN frame passes the filter in both forms (ReLU clears the NaN patch, and a NaN corner fails no comparison): its rows must agree bit for bit,
    # every other row within the bars
    fin = torch.isfinite(o0["LAFs"][:n]).flatten(1).all(dim=1)
    assert int((~fin).sum()) <= 1
    for k in ("LAFs", "descriptors"):
        assert _bits_equal(o1[k][:n][~fin], o0[k][:n][~fin]), "non-finite row: " + k
    dl = float((o1["LAFs"][:n][fin] - o0["LAFs"][:n][fin]).abs().max())
    dd = float((o1["descriptors"][:n][fin] - o0["descriptors"][:n][fin]).abs().max())
    print("rows %d (%d with a non-finite frame), recomputed %d; form 1 - form 0: LAFs max %.3g px, descriptors max %.3g; A of the constant patch %s, of the NaN frame %s"
          % (n, int((~fin).sum()), recomputed, dl, dd, A1[3].tolist(), A1[7].tolist()))
    assert dl <= 1e-3 and dd <= 1e-3
    assert (A1[7].view(np.uint32) == A0[7].view(np.uint32)).all()          # a NaN corner is never certain: recomputed by the direct kernel
    assert float(np.abs(A1[3].astype(np.float64) - A0[3]).max()) <= sm.DELTA
    assert recomputed >= 1
