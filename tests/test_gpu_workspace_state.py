"""Results of the fused calls must not depend on what the workspace, a scratch buffer or an output buffer held before the call.

Every fused entry point works inside one caller-owned workspace of which only a handful of areas are cleared per call (the
ledger and who writes what); the rest is right only because some kernel writes each byte before another reads it.  Here every call runs on a
context re-bound between guard bands (tests/_workspace_state.py), into guard-banded outputs filled with 0xFF bytes, behind these prior states of
the workspace: zeros; whatever a complete call on a denser (rich), a sparser (poor) or the same image left behind on this very context; NaN bit
patterns in every float area (integer, byte and record areas only ever hold zeros or the library's own bytes).  Asserted for every (prior state,
target) pair: the result - count, overflow flag, counters 1 .. 4 and every output array in full - equals the result from zeros BIT FOR BIT, rows
>= count of every output are zero bytes, every guard band is intact, the overflow flag is 0.  No tolerance anywhere: every comparison is on bytes.
Asserted first: two calls from zeros agree (else the rest would be inconclusive).  240 x 320, 300 features, B <= 3."""
import ctypes as C

import numpy as np
import pytest
import torch

import _workspace_state as ws

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_FRAMES = 40


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
def probes():
    return ws.load_probes()


@pytest.fixture(scope="module")
def imgs():
    return {k: f().to(DEV) for k, f in ws.IMAGES.items()}


def _extractor(amd, nets, **kw):
    attrs = {k: kw.pop(k) for k in ("lazy_shape_rows", "shape_form", "desc_form", "max_keep") if k in kw}
    args = dict(mrSize=ws.MR_SIZE, num_features=ws.N_FEATURES, border=ws.BORDER, num_Baum_iters=1, AffNet=nets[0], OriNet=nets[1])
    args.update(kw)
    det = amd.ScaleSpaceAffinePatchExtractor(**args).to(DEV)
    for k, v in attrs.items():
        setattr(det, k, v)
    return det


class Case(object):
    """An extractor whose context is re-bound between guard bands before its first call, and the caller's buffers of its calls"""

    def __init__(self, probes, det, x, ctx=None):
        self.det = det
        self.ctx = ctx if ctx is not None else det._context(x, allow_batch=True)
        self.g = ws.Guarded(probes, self.ctx)
        self.B, self.F = self.ctx.batch, self.ctx.cap_final
        self.outs = ws.Outputs(self.B, self.F, self.ctx.device)

    def run(self, img, do_ori=True, desc=None):
        if self.ctx is self.det._ctx:            # (applies the extractor's call-time switches: arithmetic, shape form, descriptor form)
            assert self.det._context(img, allow_batch=True) is self.ctx, "the extractor replaced its context: the guard bands are gone"
        nets = self.det._nets(self.ctx.device, do_ori, desc)
        return ws.extract(self.ctx, nets, img, do_ori, self.outs, desc is not None)

    def check(self, r, what):
        assert self.g.intact() and self.outs.intact(), "%s: a guard band was written" % what
        assert not r["counter0"].any(), "%s: overflow flag %s" % (what, r["counter0"])
        bad = ws.rows_past_count_are_zero(r, self.B, self.F)
        assert not bad, "%s: not zero: %s" % (what, bad)

    def close(self):
        self.g.free()
        self.outs = None
        if self.det is not None and self.ctx is self.det._ctx:
            self.det._ctx = self.det._ctx_key = None
        self.ctx = None
        torch.cuda.empty_cache()


def _same(got, ref, what):
    bad = ws.same_result(got, ref)
    assert not bad, "%s: differs from the zero-state result in: %s" % (what, bad)


def _zero_state(case, call, what):
    """The reference of a target: its result from the zero state, twice (the precondition of everything else)"""
    case.g.zero()
    ref = call()
    case.g.zero()
    again = call()
    bad = ws.same_result(again, ref)
    assert not bad, "%s: two calls from the zero state differ in %s - the call is not deterministic, nothing about prior states can be concluded" % (what, bad)
    case.check(ref, what + " from zeros")
    return ref


def _sweep(case, targets, priors, call, label, extra=None):
    """targets: {name: image}.  priors: names of `targets` (or of `extra`, images that are no targets) to run first (a stale state), 'same', or 'nan'.
    Returns the number of pairs compared."""
    pairs = 0
    stale = dict(targets, **(extra or {}))
    for tname, timg in targets.items():
        ref = _zero_state(case, lambda: call(timg), "%s, %s" % (label, tname))
        for p in priors:
            case.g.zero()
            if p == "nan":
                case.g.nan_floats()
            else:
                call(timg if p == "same" else stale[p])
            what = "%s, %s behind %s" % (label, tname, "NaN floats" if p == "nan" else "stale " + p)
            got = call(timg)
            case.check(got, what)
            _same(got, ref, what)
            pairs += 1
    return pairs


# ---- 1. the default extractor ----------------------------------------------------------------------------------------------------------------------
def test_default_extractor_behind_every_prior_state(amd, nets, probes, imgs):
    Hn = nets[2]
    # the anchor to every other test: the untouched extractor (its own torch.empty workspace and outputs)
    plain = _extractor(amd, nets)
    anchor = {}
    for name, img in imgs.items():
        r = plain.enqueue(img, do_ori=True, desc=Hn)
        torch.cuda.synchronize()
        anchor[name] = {k: r[k].contiguous().view(-1).view(torch.uint8).cpu().numpy().copy() for k in ("LAFs", "responses", "ids", "descriptors")}
        anchor[name]["count"] = r["count"].cpu().numpy().copy()
    del plain
    det = _extractor(amd, nets)
    case = Case(probes, det, imgs["rich"])
    refs = {}

    def call(img):
        return case.run(img, True, Hn)
    # (busy: full lists AND a second lazy pass - the one prior that leaves verdicts of evaluated rows where rich and poor leave "skipped" or nothing)
    pairs = _sweep(case, imgs, ("rich", "poor", "same", "nan", "busy"), call, "default", extra={"busy": ws.busy_image().to(DEV)})
    for name, img in imgs.items():
        case.g.zero()
        refs[name] = call(img)
        for k in ("LAFs", "responses", "ids", "descriptors"):
            assert refs[name][k].tobytes() == anchor[name][k].tobytes(), "%s: %s differs from what the untouched extractor returns" % (name, k)
        assert (refs[name]["count"] == anchor[name]["count"]).all()
    # the images do on the device what they were built for
    assert refs["rich"]["count"][0] == ws.N_FEATURES and refs["rich"]["counter1"][0] == ws.N_PREFILTER
    assert refs["rich"]["counter3"][0] == ws.LAZY_ROWS, "rich: the second lazy pass ran (%d candidates evaluated)" % refs["rich"]["counter3"][0]
    assert 1 <= refs["poor"]["count"][0] <= 75 and refs["poor"]["counter3"][0] == refs["poor"]["counter1"][0] < ws.N_PREFILTER
    # flat: nothing detected, every output zero, the read-back answers EMPTY
    flat = refs["flat"]
    assert flat["count"][0] == 0 and not any(flat[k].any() for k in ("LAFs", "responses", "ids", "descriptors")) and flat["counter1"][0] == 0
    with pytest.raises(amd._lib.AffnetEmptyError):
        case.ctx.read_counts()
    print("case 1: %d (prior state, target) pairs; rows rich %d poor %d flat %d" % (pairs, refs["rich"]["count"][0], refs["poor"]["count"][0], flat["count"][0]))
    case.close()


# ---- 2. call-time switches in a chain on one context ----------------------------------------------------------------------------------------------
# a variant = the default call with one switch changed: (do_ori, descriptors, shape form, descriptor form, arithmetic, AffNet weights in the device buffer)
DEFAULT = dict(do_ori=True, desc=True, shape_form=1, desc_form=4, arith="fp32", weights=0)
VARIANTS = [dict(DEFAULT), dict(DEFAULT, do_ori=False), dict(DEFAULT, desc=False), dict(DEFAULT, shape_form=0), dict(DEFAULT, shape_form=2),
            dict(DEFAULT, desc_form=0), dict(DEFAULT, desc_form=1), dict(DEFAULT, desc_form=2), dict(DEFAULT, desc_form=3),
            dict(DEFAULT, arith="fp32_split3"), dict(DEFAULT, arith="fp32_split2h"), dict(DEFAULT, weights=1)]
# The step order, fixed: a primer, then every variant once with the images alternating rich, poor, ..., then every variant again in the order
# 1, 2, ..., 11, 0 with the images still alternating - so each variant runs once directly behind rich and once directly behind poor, always behind
# another variant on the other image.
CHAIN = [(11, "poor")] + [(k % 12, ("rich", "poor")[k % 2]) for k in range(12)] + [((k + 1) % 12, ("rich", "poor")[k % 2]) for k in range(12, 24)]


def test_chain_is_what_its_comment_says():
    behind = {}
    for (pv, pi), (v, i) in zip(CHAIN[:-1], CHAIN[1:]):
        assert pv != v and pi != i
        behind.setdefault(v, set()).add(pi)
    assert behind == {v: {"rich", "poor"} for v in range(len(VARIANTS))}
    for key in DEFAULT:        # every value of every switch occurs
        assert {str(v[key]) for v in VARIANTS} >= {str(x) for x in {"do_ori": (True, False), "desc": (True, False), "shape_form": (0, 1, 2),
                                                                   "desc_form": (0, 1, 2, 3, 4), "arith": ("fp32", "fp32_split3", "fp32_split2h"),
                                                                   "weights": (0, 1)}[key]}


def test_call_time_switches_in_a_chain(amd, nets, probes, imgs, weights):
    A, O, Hn = nets
    blob = A.packed_weights(torch.device(DEV))                      # THE device buffer the calls read AffNet from: rewritten in place below
    other = {k: v.clone() for k, v in weights["AffNet"].items()}
    other["features.19.weight"] = other["features.19.weight"] * 0.5
    from affnet_amd import _lib, engine
    blobs = [blob.clone(), engine.pack_state_dict(_lib.NET_AFFNET, other, winograd=True).to(DEV)]
    assert blobs[1].shape == blob.shape and not torch.equal(blobs[0], blobs[1])

    def run(case, v, img):
        s = VARIANTS[v]
        blob.copy_(blobs[s["weights"]])
        case.det.shape_form, case.det.desc_form, case.det.arith = s["shape_form"], s["desc_form"], s["arith"]
        return case.run(img, s["do_ori"], Hn if s["desc"] else None)
    try:
        refs = {}
        for v, name in sorted(set(CHAIN)):                           # one fresh zeroed context per (variant, image), one alive at a time
            case = Case(probes, _extractor(amd, nets), imgs[name])
            refs[(v, name)] = run(case, v, imgs[name])
            case.check(refs[(v, name)], "variant %d on %s, fresh context" % (v, name))
            case.close()
        assert ws.same_result(refs[(0, "rich")], refs[(11, "rich")]) != "", "rewriting the weights in place changed nothing"
        case = Case(probes, _extractor(amd, nets), imgs["rich"])
        prev = "zeros"
        for step, (v, name) in enumerate(CHAIN):
            what = "step %d: variant %d %s on %s behind %s" % (step, v, VARIANTS[v], name, prev)
            got = run(case, v, imgs[name])
            case.check(got, what)
            bad = ws.same_result(got, refs[(v, name)])
            assert not bad, "%s: differs from a fresh zeroed context in: %s" % (what, bad)
            prev = "variant %d on %s" % (v, name)
        case.close()
        print("case 2: %d chained steps compared with %d fresh contexts" % (len(CHAIN), len(refs)))
    finally:
        blob.copy_(blobs[0])


# ---- 3. create-time variants -------------------------------------------------------------------------------------------------------------------------
CREATE = {"lazy_default": dict(lazy_shape_rows=-1), "lazy_100": dict(lazy_shape_rows=100), "lazy_off": dict(lazy_shape_rows=0),
          "baum_3": dict(num_Baum_iters=3), "handcrafted_19px": dict(AffNet=None, OriNet=None), "nlevels_4": dict(nlevels=4),
          "threshold": dict(th=50.0, max_keep=4096)}


@pytest.mark.parametrize("variant", sorted(CREATE))
def test_create_time_variants(amd, nets, probes, imgs, variant):
    Hn = nets[2]
    det = _extractor(amd, nets, **CREATE[variant])
    case = Case(probes, det, imgs["rich"])
    if variant == "nlevels_4":
        assert any(a["name"] == "octave_map" and a["cleared"] for a in case.g.areas), "this variant is here for the octaveMap path"
    pairs = _sweep(case, imgs, ("rich", "poor"), lambda img: case.run(img, True, Hn), variant)
    print("case 3 %s: %d pairs" % (variant, pairs))
    case.close()


# ---- 4. a batch of three ---------------------------------------------------------------------------------------------------------------------------
def test_batch_slots_behind_denser_and_sparser_predecessors(amd, nets, probes, imgs):
    Hn = nets[2]
    names = ("rich", "poor", "flat")
    single = {}
    for n in names:                                                  # three single-image contexts, each fresh and zeroed, one alive at a time
        case = Case(probes, _extractor(amd, nets), imgs[n])
        single[n] = case.run(imgs[n], True, Hn)
        case.check(single[n], "single " + n)
        case.close()
    rot = [names[k:] + names[:k] for k in range(3)]
    batch = [torch.cat([imgs[n] for n in r]).contiguous() for r in rot]
    case = Case(probes, _extractor(amd, nets), batch[0])
    pairs = 0
    for k in range(3):
        ref = _zero_state(case, lambda: case.run(batch[k], True, Hn), "batch %s" % (rot[k],))
        case.g.zero()
        case.run(batch[k - 1], True, Hn)
        got = case.run(batch[k], True, Hn)
        what = "batch %s behind %s" % (rot[k], rot[k - 1])
        case.check(got, what)
        _same(got, ref, what)
        pairs += 1
        F = case.F
        for b, n in enumerate(rot[k]):                               # each slot equals the single-image call, bit for bit
            s = single[n]
            for key in ("count", "counter0", "counter1", "counter2", "counter3", "counter4"):
                assert got[key][b] == s[key][0], (what, b, key)
            for key, (w, _) in ws.Outputs.SHAPES.items():
                assert got[key].reshape(3, F * w * 4)[b].tobytes() == s[key].tobytes(), "%s: slot %d (%s): %s differs from the single-image call" % (what, b, n, key)
    print("case 4: %d pairs" % pairs)
    case.close()


# ---- 5. caller frames behind a detection and the reverse -------------------------------------------------------------------------------------------
def _frames():
    """40 pixel frames on a grid, sizes 6 .. 20 px, mildly anisotropic and rotated"""
    k = torch.arange(N_FRAMES, dtype=torch.float32)
    cx, cy = 40.0 + 30.0 * (k % 8), 40.0 + 35.0 * torch.div(k, 8, rounding_mode="floor")
    s, ang = 6.0 + 0.35 * k, 0.3 * k
    a, b = s * torch.cos(ang), -0.8 * s * torch.sin(ang)
    c, d = s * torch.sin(ang), 0.8 * s * torch.cos(ang)
    return torch.stack([torch.stack([a, b, cx], 1), torch.stack([c, d, cy], 1)], 1).contiguous().to(DEV)


def test_caller_frames_and_detection_share_a_context(amd, nets, probes, imgs):
    from affnet_amd import engine
    from affnet_amd._lib import lib, check
    Hn, img, frames = nets[2], imgs["rich"], _frames()

    def fresh():
        det = _extractor(amd, nets)
        return Case(probes, det, img, ctx=det._frames_context(img, N_FRAMES))

    def describe(case):
        n = case.det._nets(case.ctx.device, True, Hn)
        case.outs.poison()
        o = case.outs
        check(lib.affnet_describe_frames(case.ctx.handle, C.byref(n), C.c_void_p(img.data_ptr()), C.c_void_p(frames.data_ptr()), None, None, N_FRAMES, 1,
                                         o.ptr("LAFs"), o.ptr("responses"), o.ptr("ids"), o.ptr("descriptors"), o.ptr("count"), engine.stream_of(case.ctx.device)),
              case.ctx.handle, "affnet_describe_frames")
        return ws.collect(case.ctx, o, True)
    case = fresh()
    assert case.ctx.cap_pre == N_FRAMES
    ref_frames = _zero_state(case, lambda: describe(case), "describe_frames")
    assert 1 <= ref_frames["count"][0] <= N_FRAMES
    case.close()
    case = fresh()
    ref_detect = _zero_state(case, lambda: case.run(img, True, Hn), "detection on the frames context")
    case.close()
    case = fresh()
    case.run(img, True, Hn)
    for step, (call, ref, what) in enumerate([(lambda: describe(case), ref_frames, "describe_frames behind a detection"),
                                              (lambda: case.run(img, True, Hn), ref_detect, "detection behind describe_frames"),
                                              (lambda: describe(case), ref_frames, "describe_frames behind a detection, again")]):
        got = call()
        case.check(got, what)
        _same(got, ref, what)
    print("case 5: 3 pairs; %d of %d frames survive the shape filter" % (ref_frames["count"][0], N_FRAMES))
    case.close()


# ---- 6. OnePassSIR -----------------------------------------------------------------------------------------------------------------------------------
def test_onepass_context(amd, nets, probes, imgs, weights):
    from affnet_amd import _lib, engine
    from affnet_amd._lib import lib, check
    A, O, Hn = nets
    FC = amd.AffNetFastFullConv(); FC.load_state_dict(weights["AffNet"]); FC = FC.to(DEV)
    sir = amd.OnePassSIR(mrSize=ws.MR_SIZE, num_features=ws.N_FEATURES, border=15, AffNet=FC, OriNet=O).to(DEV)
    case = Case(probes, None, None, ctx=sir._context(imgs["rich"]))
    dev = case.ctx.device
    n = _lib.Nets()
    n.d_orinet, n.d_hardnet = O.packed_weights(dev).data_ptr(), Hn.packed_weights(dev).data_ptr()
    packed = FC.packed_weights(dev)

    def call(img, maps=None):
        st, o = engine.stream_of(dev), case.outs
        if maps is not None:                                         # the slot for a foreign dense AffNet: the caller writes the maps, the library reads them
            check(lib.affnet_pyramid_build(case.ctx.handle, C.c_void_p(img.data_ptr()), st), case.ctx.handle, "affnet_pyramid_build")
            for view in case.ctx.affmap_views(0):
                view.copy_(maps.view(1, 4, 1, 1).expand_as(view))
            check(lib.affnet_detect_image_onepass(case.ctx.handle, None, None, st), case.ctx.handle, "affnet_detect_image_onepass")
        else:
            check(lib.affnet_detect_image_onepass(case.ctx.handle, C.c_void_p(packed.data_ptr()), C.c_void_p(img.data_ptr()), st), case.ctx.handle,
                  "affnet_detect_image_onepass")
        o.poison()
        check(lib.affnet_describe_detected(case.ctx.handle, C.byref(n), 1, o.ptr("LAFs"), o.ptr("responses"), o.ptr("ids"), o.ptr("descriptors"),
                                           o.ptr("count"), st), case.ctx.handle, "affnet_describe_detected")
        return ws.collect(case.ctx, o, True)
    pairs = _sweep(case, imgs, ("rich", "poor"), call, "OnePassSIR")
    case.g.zero()
    assert call(imgs["rich"])["count"][0] > 0
    # caller-written maps behind calls that computed theirs
    maps = torch.tensor([1.1, 0.0, 0.2, 0.9], device=DEV)
    ref = _zero_state(case, lambda: call(imgs["rich"], maps), "caller-written maps")
    assert ref["count"][0] > 0
    for p in ("rich", "poor"):
        case.g.zero()
        call(imgs[p])
        what = "caller-written maps behind computed maps of " + p
        got = call(imgs["rich"], maps)
        case.check(got, what)
        _same(got, ref, what)
        pairs += 1
    print("case 6: %d pairs" % pairs)
    case.close()


# ---- 7. graph replay ---------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_on_a_poisoned_workspace(amd, nets, probes, imgs):
    from affnet_amd import engine
    from affnet_amd._lib import lib, check
    Hn = nets[2]
    det = _extractor(amd, nets)
    case = Case(probes, det, imgs["rich"])
    eager = _zero_state(case, lambda: case.run(imgs["rich"], True, Hn), "eager")
    n = det._nets(case.ctx.device, True, Hn)
    static = imgs["rich"].clone()
    stream = torch.cuda.Stream(device=DEV)
    case.g.zero()                                                    # captured on the zero state; nothing runs during the capture
    torch.cuda.synchronize()
    o = case.outs
    check(lib.affnet_graph_capture_extract(case.ctx.handle, C.byref(n), C.c_void_p(static.data_ptr()), 1, o.ptr("LAFs"), o.ptr("responses"), o.ptr("ids"),
                                           o.ptr("descriptors"), o.ptr("count"), C.c_void_p(stream.cuda_stream)), case.ctx.handle, "affnet_graph_capture_extract")

    def replay(img):
        static.copy_(img)
        o.poison()
        check(lib.affnet_graph_launch(case.ctx.handle, engine.stream_of(case.ctx.device)), case.ctx.handle, "affnet_graph_launch")
        return ws.collect(case.ctx, o, True)
    got = replay(imgs["rich"])
    case.check(got, "replay from zeros")
    _same(got, eager, "replay from zeros")
    replay(imgs["poor"])                                             # stale poor, left by a replay
    for what, prepare in (("replay behind a replay of poor", lambda: None), ("replay behind NaN floats", case.g.nan_floats)):
        prepare()
        got = replay(imgs["rich"])
        case.check(got, what)
        _same(got, eager, what)
    print("case 7: 3 replays compared with the eager call")
    case.close()


# ---- 8. stand-alone calls whose scratch the caller owns ----------------------------------------------------------------------------------------------
def _scratch_pair(nbytes_scratch, nbytes_out, launch, what):
    """launch(scratch pointer, out pointer) with the scratch full of 0xFF bytes and full of zeros: the same output bytes, guard bands intact"""
    scratch, out = ws.Banded(nbytes_scratch, DEV), ws.Banded(nbytes_out, DEV)
    res = []
    for fill in (0xFF, 0x00):
        scratch.mid.fill_(fill)
        out.mid.fill_(0xFF)
        launch(C.c_void_p(scratch.mid.data_ptr()), C.c_void_p(out.mid.data_ptr()))
        torch.cuda.synchronize()
        assert scratch.intact() and out.intact(), "%s: a guard band was written" % what
        res.append(out.mid.cpu().numpy().copy())
    assert res[0].tobytes() == res[1].tobytes(), "%s: the output depends on what the scratch held" % what
    assert np.isfinite(res[0].view(np.float32)).all(), "%s: output bytes never written" % what


def _patches(n):
    g = torch.Generator().manual_seed(100 + n)
    return torch.rand(n, 32, 32, generator=g).to(DEV).contiguous()


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("arith", ["fp32", "fp32_split3", "fp32_split2h"])
def test_cnn32_forward_scratch(amd, nets, n, arith):
    from affnet_amd import _lib, engine
    from affnet_amd._lib import lib, check
    dev = torch.device(DEV)
    x = _patches(n)
    for kind, net in zip((_lib.NET_AFFNET, _lib.NET_ORINET, _lib.NET_HARDNET), nets):
        packed = net.packed_weights(dev)
        ctx = engine.utility_ctx(dev, arith)
        hard = kind == _lib.NET_HARDNET

        def launch(scratch, out):
            check(lib.affnet_cnn32_forward(ctx, kind, C.c_void_p(packed.data_ptr()), C.c_void_p(x.data_ptr()), None, n, out, scratch, engine.stream_of(dev)),
                  ctx, "affnet_cnn32_forward")
        _scratch_pair(n * ((8192 + 512) if hard else 144) * 4, n * (128 if hard else 4) * 4, launch, "cnn32_forward net %d %s n %d" % (kind, arith, n))


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("form", ["c5", "c1"])
def test_hardnet_four_patch_conv5_scratch(amd, nets, probes, n, form):
    """Descriptor forms 3 / 4 (the fused default) on patch tensors, through the probe library: n = 5 is one full group of the four-patch conv5 kernel and
    a tail group of one"""
    from affnet_amd import _lib, engine
    dev = torch.device(DEV)
    fn = getattr(probes, "affnet_probe_hardnet_%s_forward" % form)
    fn.restype, fn.argtypes = _lib.PROBE_SYMBOLS["affnet_probe_hardnet_%s_forward" % form]
    x, packed, ctx = _patches(n), nets[2].packed_weights(dev), engine.utility_ctx(dev, "fp32")

    def launch(scratch, out):
        assert fn(ctx, C.c_void_p(packed.data_ptr()), C.c_void_p(x.data_ptr()), n, out, scratch, engine.stream_of(dev)) == 0
    _scratch_pair(n * (8192 + 512) * 4, n * 128 * 4, launch, "hardnet form %s n %d" % (form, n))


@pytest.mark.parametrize("h,w", [(34, 34), (65, 97), (100, 70)])
def test_fullconv_forward_scratch(amd, weights, h, w):
    from affnet_amd import engine
    from affnet_amd._lib import lib, check
    dev = torch.device(DEV)
    FC = amd.AffNetFastFullConv(); FC.load_state_dict(weights["AffNet"]); FC = FC.to(DEV)
    packed, ctx = FC.packed_weights(dev), engine.utility_ctx(dev, "fp32")
    g = torch.Generator().manual_seed(h * 1000 + w)
    img = (torch.rand(1, 1, h, w, generator=g) * 255.0).to(DEV).contiguous()

    def launch(scratch, out):
        check(lib.affnet_fullconv_forward(ctx, C.c_void_p(packed.data_ptr()), C.c_void_p(img.data_ptr()), h, w, out, scratch, engine.stream_of(dev)), ctx,
              "affnet_fullconv_forward")
    _scratch_pair(lib.affnet_fullconv_scratch_bytes(h, w), 4 * h * w * 4, launch, "fullconv_forward %dx%d" % (h, w))


@pytest.mark.parametrize("n", [1, 65])
def test_tfeat_forward_scratch(amd, n):
    from affnet_amd import engine
    from affnet_amd._lib import lib, check
    dev = torch.device(DEV)
    torch.manual_seed(0)
    net = amd.HardTFeatNet(None).to(DEV)
    packed, ctx, x = net.packed_weights(dev), engine.utility_ctx(dev, "fp32"), _patches(n)

    def launch(scratch, out):
        check(lib.affnet_tfeat_forward(ctx, C.c_void_p(packed.data_ptr()), C.c_void_p(x.data_ptr()), None, n, out, scratch, engine.stream_of(dev)), ctx,
              "affnet_tfeat_forward")
    _scratch_pair(lib.affnet_tfeat_scratch_floats(n) * 4, n * 128 * 4, launch, "tfeat_forward n %d" % n)
