"""The stride-2 layers conv2 / conv4 of the 16-channel trunks as polyphase Winograd F(2x2, 2x2) (affnet_amd/csrc/cnn_mfma.h: conv3x3_poly16_mfma_rows,
poly16_combine): in the first AffNet trunk of shape form 2 (cnn32_trunk_kernel<AffNet, 8, *, 5>; selectable, form 1 stays the default; reached on patch tensors through libaffnet_hip_probes.so:
affnet_probe_affnet_poly_*) and in the one exact OriNet trunk (what OriNetFast.forward and affnet_cnn32_debug_layer run).  Their 25-position weights are derived from
the blob's BN-folded taps by wino_derive_u_kernel in front of every launch, behind the Winograd sections of the context's buffer.
Pinned here: the derived U bit for bit (shipped blobs and seeded weights), layers 2 and 4 of both kernels against a torch CPU forward within the OriNet layer bar
5e-5 * max(1, |ref|max) - shipped weights, the nine single-tap states of either layer, a patch that is non-zero only on its outermost ring - batches of 1, 2 and 17
patches and a second run bit for bit, shape form 2 against form 0 on three 320x240 images (counts, ids, responses bit-equal, flagged rows with the direct kernel's A,
|dA| <= 4e-6 elsewhere) with both lazy settings, graph replay against eager, and that a blob rewritten in place never meets stale U."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _shape_margin as sm  # noqa: E402
import affnet_oracle as orc  # noqa: E402
import winograd_numerics as wn  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NETS = [(0, "AffNet"), (1, "OriNet")]
SEEDS = (0, 1, 2)
KEYS = ("LAFs", "responses", "ids", "descriptors", "count")
CONV_OF_LAYER = {li: ci for li, (ci, bi, st) in enumerate(orc._TRUNK)}


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return affnet_amd


@pytest.fixture(scope="module")
def probes():
    from affnet_amd import _lib
    assert os.path.isfile(_lib.PROBES_LIB_PATH), "libaffnet_hip_probes.so is missing (AFFNET_PROBES=1 bash affnet_amd/csrc/build.sh)"
    pl = C.CDLL(_lib.PROBES_LIB_PATH)
    for name in ("affnet_probe_affnet_poly_layer", "affnet_probe_affnet_poly_partials", "affnet_probe_trunk16_poly_u", "affnet_probe_shape_offsets"):
        getattr(pl, name).restype, getattr(pl, name).argtypes = _lib.PROBE_SYMBOLS[name]
    return pl


def _net(amd, kind, sd):
    net = (amd.AffNetFast if kind == 0 else amd.OriNetFast)(PS=32)
    net.load_state_dict(sd)
    return net.to(DEV)


def _seeded_state(sd, seed):
    """Seeded random weights and BatchNorm statistics of the shapes of `sd`, unrelated to the shipped ones"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if not torch.is_floating_point(v):
            out[k] = v.clone()
        elif k.endswith("running_var"):
            out[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("weight"):
            out[k] = torch.randn(v.shape, generator=g) / float(v[0].numel()) ** 0.5
        else:
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
    return out


def _second_weights(sd, seed=21):
    """A second set of weights of the same shapes: every conv kernel perturbed by seeded noise of 10 % of its own spread (the network still finds its 300 shapes)"""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    for i in (0, 3, 6, 9, 12, 15):
        w = out["features.%d.weight" % i]
        out["features.%d.weight" % i] = w + 0.1 * w.std() * torch.randn(w.shape, generator=g)
    return out


def _torch_layers(sd, p):
    """The reference trunk on the CPU: conv, eval BatchNorm (affine=False), ReLU; the six layers' outputs of the one patch"""
    outs = []
    with torch.no_grad():
        x = orc.input_norm(p)
        for ci, bi, st in orc._TRUNK:
            x = F.conv2d(x, sd["features.%d.weight" % ci], None, stride=st, padding=1)
            x = F.relu(F.batch_norm(x, sd["features.%d.running_mean" % bi], sd["features.%d.running_var" % bi], None, None, False, 0.1, 1e-5))
            outs.append(x[0])
    return outs


def _patch(seed=5):
    return torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(seed)) * 255


def _ring_patch():
    p = torch.zeros(1, 1, 32, 32)
    r = _patch(6)
    for sl in ((0, 0, 0), (0, 0, 31), (0, 0, slice(None), 0), (0, 0, slice(None), 31)):
        p[sl] = r[sl]
    return p


def _dump(amd, probes, kind, sd, p, layer, numel):
    """Layer dump of the polyphase kernel of net `kind`: AffNet through the probe of shape form 2's trunk, OriNet through the product library's debug entry"""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    packed = _net(amd, kind, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    out = torch.zeros(numel, device=DEV)
    pd = p[0, 0].to(DEV).contiguous()
    if kind == 0:
        check(probes.affnet_probe_affnet_poly_layer(ctx, 0, ptr(packed), ptr(pd), layer, ptr(out), None), ctx, "probe_affnet_poly_layer")
    else:
        check(lib.affnet_cnn32_debug_layer(ctx, 1, ptr(packed), ptr(pd), layer, ptr(out), None), ctx, "debug_layer")
    torch.cuda.synchronize()
    return out.cpu()


def _check_layer(got, ref, layer, what):
    """bar of test_orinet_trunk_layer_by_layer; names the worst (tile block, channel block) of the layer's 2x2 output tiles"""
    d = (got.reshape(ref.shape).double() - ref.double()).abs()
    bar = 5e-5 * max(1.0, float(ref.abs().max()))
    c, y, x = np.unravel_index(int(d.argmax()), d.shape)
    ht = ref.shape[-1] // 2
    print("%s layer %d %s: max abs diff %.3g (|ref|max %.3g, bar %.3g) at channel %d pixel (%d, %d)" % (what, layer, tuple(ref.shape), float(d.max()), float(ref.abs().max()), bar, c, y, x))
    assert float(d.max()) < bar, "%s layer %d: %.3g at tile block %d, channel block %d (channel %d, pixel (%d, %d))" % (
        what, layer, float(d.max()), ((y // 2) * ht + x // 2) // 16, c // 16, c, y, x)


def _partials(probes, packed, p):
    """Head partials (n, 32) of shape form 2's first trunk on (n, 1, 32, 32) patches on the device"""
    from affnet_amd import engine
    from affnet_amd._lib import ptr, check
    ctx = engine.utility_ctx(torch.device(DEV))
    n = p.shape[0]
    x = p[:, 0].contiguous().float()
    out = torch.zeros(n * 32, device=DEV)
    check(probes.affnet_probe_affnet_poly_partials(ctx, ptr(packed), ptr(x), n, ptr(out), None), ctx, "probe_affnet_poly_partials")
    torch.cuda.synchronize()
    return out.view(n, 32)


@pytest.mark.parametrize("state", ["shipped", "seeded"])
@pytest.mark.parametrize("kind,name", NETS)
def test_derived_u_is_bitwise_the_mirror(amd, probes, weights, kind, name, state):
    from affnet_amd import engine
    from affnet_amd._lib import ptr, check
    sd = weights[name] if state == "shipped" else _seeded_state(weights[name], 7 + kind)
    packed = _net(amd, kind, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    want = wn.poly16_packed_weight_transform(sd)
    for layer, size in ((2, 25 * 16 * 32), (4, 25 * 32 * 64)):
        w = want[layer].numpy()
        assert w.size == size
        out = torch.zeros(w.size, device=DEV)
        check(probes.affnet_probe_trunk16_poly_u(ctx, kind, ptr(packed), layer, ptr(out), None), ctx, "probe_trunk16_poly_u")
        torch.cuda.synchronize()
        bad = int((out.cpu().numpy().view(np.uint32) != w.view(np.uint32)).sum())
        print("%s %s conv%d: %d of %d derived U values differ from the mirror" % (name, state, layer, bad, w.size))
        assert bad == 0


@pytest.mark.parametrize("kind,name", NETS)
def test_layers_2_and_4_against_torch(amd, probes, weights, kind, name):
    for what, sd in (("shipped " + name, weights[name]), ("seeded " + name, _seeded_state(weights[name], 17 + kind))):
        p = _patch()
        want = _torch_layers(sd, p)
        for layer in (2, 4):
            _check_layer(_dump(amd, probes, kind, sd, p, layer, want[layer].numel()), want[layer], layer, what)


@pytest.mark.parametrize("layer", [2, 4])
@pytest.mark.parametrize("kind,name", NETS)
def test_single_tap_weights(amd, probes, weights, kind, name, layer):
    base = _seeded_state(weights[name], 9 + kind)
    key = "features.%d.weight" % CONV_OF_LAYER[layer]
    p = _patch()
    for tap in range(9):
        sd = {k: v.clone() for k, v in base.items()}
        w = torch.zeros_like(sd[key])
        w[:, :, tap // 3, tap % 3] = base[key][:, :, tap // 3, tap % 3]
        sd[key] = w
        want = _torch_layers(sd, p)[layer]
        _check_layer(_dump(amd, probes, kind, sd, p, layer, want.numel()), want, layer, "%s tap (ky %d, kx %d)" % (name, tap // 3, tap % 3))


@pytest.mark.parametrize("kind,name", NETS)
def test_patch_that_is_nonzero_only_on_its_outermost_ring(amd, probes, weights, kind, name):
    p = _ring_patch()
    assert float(p[0, 0, 1:31, 1:31].abs().max()) == 0.0 and float(p.abs().max()) > 0
    want = _torch_layers(weights[name], p)
    for layer in (2, 4):
        _check_layer(_dump(amd, probes, kind, weights[name], p, layer, want[layer].numel()), want[layer], layer, "%s ring patch" % name)


@pytest.fixture(scope="module")
def batch():
    g = np.load(os.path.join(ROOT, "tests", "golden", "cnn_random_patches.npz"))
    p = torch.from_numpy(g["patches"]).reshape(-1, 1, 32, 32)
    extra = torch.rand(max(0, 20 - p.shape[0]), 1, 32, 32, generator=torch.Generator().manual_seed(3)) * 255
    return torch.cat([p, extra])[:20].to(DEV)


def test_affnet_batches_of_1_2_17_and_a_second_run_give_the_same_bits(amd, probes, weights, batch):
    packed = _net(amd, 0, weights["AffNet"]).packed_weights(torch.device(DEV))
    whole = _partials(probes, packed, batch).clone()
    assert torch.equal(whole, _partials(probes, packed, batch)), "a second run changed the partials"
    assert float(whole.abs().max()) > 0
    at = 0
    for n in (1, 2, 17):
        assert torch.equal(_partials(probes, packed, batch[at:at + n]), whole[at:at + n]), "batch of %d" % n
        at += n


def test_orinet_batches_of_1_2_17_and_a_second_run_give_the_same_bits(amd, weights, batch):
    net = _net(amd, 1, weights["OriNet"])
    whole = net(batch).clone()
    assert torch.equal(whole, net(batch)), "a second run changed the angles"
    at = 0
    for n in (1, 2, 17):
        assert torch.equal(net(batch[at:at + n]), whole[at:at + n]), "batch of %d" % n
        at += n


def test_affnet_blob_rewritten_in_place_is_used_by_the_next_form2_call(amd, probes, weights, batch):
    dev = torch.device(DEV)
    A1, A2 = _net(amd, 0, weights["AffNet"]), _net(amd, 0, _seeded_state(weights["AffNet"], 13))
    p = batch[:17]
    first = _partials(probes, A1.packed_weights(dev), p).clone()
    want = _partials(probes, A2.packed_weights(dev), p).clone()
    assert not torch.equal(first, want)
    A1.packed_weights(dev).copy_(A2.packed_weights(dev))                          # same device buffer, new weights
    assert torch.equal(_partials(probes, A1.packed_weights(dev), p), want)


# ---- shape form 2 against form 0 on the fused path ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(amd, weights):
    Hn = amd.HardNet(); Hn.load_state_dict(weights["HardNet"]); Hn = Hn.to(DEV)
    return _net(amd, 0, weights["AffNet"]), _net(amd, 1, weights["OriNet"]), Hn


@pytest.fixture(scope="module")
def images():
    return torch.cat([orc.synthetic_image(sm.H, sm.W, s) for s in SEEDS]).to(DEV)


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


def _shape_rows(probes, det, x):
    """The shape pass alone (no orientation, no descriptors: they reuse the scratch the flags live in): A and flags of every candidate, the per-image counters"""
    r = det.enqueue(x, do_ori=False, desc=None)
    torch.cuda.synchronize()
    ctx = det._ctx
    B, P = ctx.batch, ctx.cap_pre
    off = (C.c_int64 * 3)()
    assert probes.affnet_probe_shape_offsets(ctx.handle, C.byref(off)) == 0
    oA, oF, oL = list(off)
    A = ctx.workspace.view(torch.float32)[oA:oA + B * P * 4].view(B, P, 4).cpu().numpy().copy()
    flags = ctx.workspace.view(torch.int32)[oF:oF + B * P].view(B, P).cpu().numpy().copy()
    lafs = ctx.workspace.view(torch.float32)[oL:oL + B * P * 6].view(B, P, 6).cpu().numpy().copy()
    return {"A": A, "flags": flags, "lafs": lafs, "evaluated": ctx.counter_view(3).cpu().numpy().copy(), "recomputed": ctx.counter_view(4).cpu().numpy().copy(),
            "out": {k: r[k].clone() for k in ("LAFs", "responses", "ids", "count")}}


def test_form2_is_selectable_and_form1_stays_the_default(amd, nets):
    from affnet_amd import engine
    from affnet_amd._lib import lib
    det = amd.ScaleSpaceAffinePatchExtractor(mrSize=sm.MR_SIZE, num_features=sm.N_FEATURES, border=sm.BORDER, num_Baum_iters=1, AffNet=nets[0], OriNet=nets[1])
    assert det.shape_form == 1
    assert lib.affnet_get_shape_form(engine.utility_ctx(torch.device(DEV))) == 1          # a fresh context: the library's default
    det.shape_form = 2
    r = det.to(DEV).enqueue(orc.synthetic_image(sm.H, sm.W, 0).to(DEV), do_ori=False, desc=None)
    torch.cuda.synchronize()
    assert det._ctx.shape_form == 2 and int(r["count"][0]) > 0


@pytest.mark.parametrize("lazy", [-1, 100])
def test_form2_decides_as_form0_and_flagged_rows_carry_the_direct_bits(amd, nets, images, probes, lazy):
    """lazy = 100: the first pass cannot reach 300 survivors, so the second pass certainly runs"""
    r0 = _shape_rows(probes, _extractor(amd, nets, 0, lazy), images)
    r2 = _shape_rows(probes, _extractor(amd, nets, 2, lazy), images)
    assert int(r0["out"]["count"].min()) > 0
    assert _bits_equal(r2["out"]["count"], r0["out"]["count"])
    for b, n in enumerate(r0["out"]["count"].tolist()):
        for k in ("ids", "responses"):
            assert _bits_equal(r2["out"][k][b, :n], r0["out"][k][b, :n]), "image %d: %s" % (b, k)
    assert (r0["evaluated"] == r2["evaluated"]).all() and (r0["recomputed"] == 0).all()
    if lazy == 100:
        assert (r2["evaluated"] > 100).all(), "the second pass did not run"
    moved = 0
    for b in range(len(SEEDS)):
        n = int(r2["evaluated"][b])
        flag = r2["flags"][b, :n] != 0
        A0, A2 = r0["A"][b, :n], r2["A"][b, :n]
        dA = np.abs(A2.astype(np.float64) - A0)
        moved += int((A2[~flag].view(np.uint32) != A0[~flag].view(np.uint32)).any(axis=1).sum())
        print("lazy %d image %d: %d evaluated, %d flagged (counter %d, %.2f %%), |dA| max on unflagged rows %.3g"
              % (lazy, b, n, int(flag.sum()), int(r2["recomputed"][b]), 100.0 * flag.mean(), float(dA[~flag].max())))
        assert (A2[flag].view(np.uint32) == A0[flag].view(np.uint32)).all(), "a flagged row does not carry the direct kernel's A"
        assert float(dA[~flag].max()) <= sm.DELTA
        assert int(flag.sum()) == int(r2["recomputed"][b])
        assert not sm.margin_flag(A2[~flag], r2["lafs"][b, :n][~flag]).any()
    assert moved > 0, "form 2 did not run another kernel"


@pytest.mark.parametrize("lazy", [-1, 100])
def test_form2_full_call_returns_form0s_rows(amd, nets, images, lazy):
    want = _full(_extractor(amd, nets, 0, lazy), images, nets[2])
    got = _full(_extractor(amd, nets, 2, lazy), images, nets[2])
    assert _bits_equal(got["count"], want["count"])
    dl = dd = 0.0
    for b, n in enumerate(want["count"].tolist()):
        for k in ("ids", "responses"):
            assert _bits_equal(got[k][b, :n], want[k][b, :n]), "image %d: %s" % (b, k)
        dl = max(dl, float((got["LAFs"][b, :n] - want["LAFs"][b, :n]).abs().max()))
        dd = max(dd, float((got["descriptors"][b, :n] - want["descriptors"][b, :n]).abs().max()))
    print("lazy %d: rows %s; form 2 - form 0: LAFs max %.3g px, descriptors max %.3g" % (lazy, want["count"].tolist(), dl, dd))
    assert dl <= 1e-3 and dd <= 1e-3          # the bars of tests/test_gpu_shape_form.py


def test_form2_under_graph_replay_equals_eager(amd, nets, images):
    Hn = nets[2]
    a = _full(_extractor(amd, nets, 2), images, Hn)
    cap = _extractor(amd, nets, 2).capture(images[:1], do_ori=True, desc=Hn)
    for i in (1, 0, 2):
        g = cap.run(images[i:i + 1])
        n = int(a["count"][i])
        for k in ("LAFs", "responses", "ids", "descriptors"):
            assert _bits_equal(g[k], a[k][i, :n]), "graph replay of image %d: %s" % (i, k)


def test_blob_rewritten_in_place_is_used_by_a_form2_graph_replay(amd, nets, weights, images):
    dev = torch.device(DEV)
    A1, A2 = _net(amd, 0, weights["AffNet"]), _net(amd, 0, _second_weights(weights["AffNet"]))
    x = images[:1]

    def run(A, graph=False):
        det = _extractor(amd, (A, nets[1], nets[2]), 2)
        return det.capture(x, do_ori=True, desc=nets[2]) if graph else det.run(x, do_ori=True, desc=nets[2])

    want1, want2 = run(A1), run(A2)
    assert not torch.equal(want1["LAFs"], want2["LAFs"])
    cap = run(A1, graph=True)
    got1 = cap.run(x)
    for k in ("LAFs", "responses", "descriptors", "ids"):
        assert torch.equal(got1[k], want1[k]), k
    A1.packed_weights(dev).copy_(A2.packed_weights(dev))                          # the graph holds this address
    got2 = cap.run(x, check_weights=False)
    for k in ("LAFs", "responses", "descriptors", "ids"):
        assert torch.equal(got2[k], want2[k]), k
