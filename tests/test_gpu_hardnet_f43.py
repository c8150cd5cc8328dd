"""Descriptor form 2: the exact HardNet trunk of form 1 with conv3 as Winograd F(4x4, 3x3) (affnet_amd/csrc/cnn_mfma.h: conv3x3_f43_mfma_shared_v + f43_combine;
cnn32_trunk_kernel<HardNet, 8, *, 4>).  The transformed weights are not part of the packed blob: f43_derive_u_kernel (affnet_amd/csrc/cnn_trunk_hardnet_f43.hip)
derives them - for conv1 as well, which the trunk still runs as F(2x2, 3x3) - from the blob's BN-folded taps in front of every form 2 trunk launch, behind the
polyphase weights in the buffer the context owns.  Pinned here: the derived U of layers 1 and 3 bit for bit, layers 1 and 3 of the kernel against a torch CPU forward
(the worst tile block / channel block / pixel named) on a seeded patch, with the nine single-tap weight states and on a patch whose live pixels are its outermost ring,
the fused descriptors of form 2 against form 0 (everything but the descriptors bit-equal), the descriptors against float64 on the ragged fixture batch at a bar taken
from the CPU mirror's own error, batch-split and run-to-run bit-equality, and that a blob rewritten in place never meets stale U - eagerly or in a replayed graph.
The patch-tensor calls go through libaffnet_hip_probes.so (affnet_probe_hardnet_f43_*): HardNet.forward always runs form 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402
import winograd_numerics as wn  # noqa: E402
from make_golden_hardnet_desc import hardnet_fixture_batch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODE_BAR = 1e-5     # the project's HardNet bar between arithmetic modes (tests/test_gpu_parity.py): the float64 bar never exceeds it
FORM = 2


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
    for name in ("affnet_probe_hardnet_f43_layer", "affnet_probe_hardnet_f43_forward", "affnet_probe_hardnet_f43_u"):
        getattr(pl, name).restype, getattr(pl, name).argtypes = _lib.PROBE_SYMBOLS[name]
    return pl


def _net(amd, sd):
    H = amd.HardNet()
    H.load_state_dict(sd)
    return H.to(DEV)


def _seeded_state(seed):
    """Seeded random weights and BatchNorm statistics of HardNet's shapes, unrelated to synthetic_hardnet_state's"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in orc.synthetic_hardnet_state(0).items():
        if k.endswith("running_var"):
            out[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("weight"):
            out[k] = torch.randn(v.shape, generator=g) / float(v[0].numel()) ** 0.5
        else:
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
    return out


def _state(name):
    return orc.synthetic_hardnet_state(0) if name == "synthetic" else _seeded_state(7)


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


def _patch():
    return torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(5)) * 255


def _ring_patch():
    """Only the outermost ring of pixels is live: what the edge tiles read next to their halo"""
    p = torch.zeros(1, 1, 32, 32)
    ring = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(6)) * 255
    for sl in ((slice(0, 1), slice(None)), (slice(31, 32), slice(None)), (slice(None), slice(0, 1)), (slice(None), slice(31, 32))):
        p[0, 0][sl] = ring[0, 0][sl]
    return p


def _dump(amd, probes, sd, p, layer, numel):
    from affnet_amd import engine
    from affnet_amd._lib import ptr, check
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    out = torch.zeros(numel, device=DEV)
    check(probes.affnet_probe_hardnet_f43_layer(ctx, ptr(packed), ptr(p[0, 0].to(DEV).contiguous()), layer, ptr(out), None), ctx, "probe_hardnet_f43_layer")
    torch.cuda.synchronize()
    return out.cpu()


def _forward(probes, packed, p):
    """Descriptors of form 2 for (n, 1, 32, 32) patches on the device, through the probe launch"""
    from affnet_amd import engine
    from affnet_amd._lib import ptr, check
    ctx = engine.utility_ctx(torch.device(DEV))
    n = p.shape[0]
    x = p[:, 0].contiguous().float()
    out = torch.empty(n, 128, device=DEV)
    scratch = torch.empty(n * (8192 + 512), device=DEV)
    check(probes.affnet_probe_hardnet_f43_forward(ctx, ptr(packed), ptr(x), n, ptr(out), ptr(scratch), None), ctx, "probe_hardnet_f43_forward")
    torch.cuda.synchronize()
    return out


def _check_layer(got, ref, layer, what):
    """the project's layer bar (test_orinet_trunk_layer_by_layer); names the worst (tile block, channel block, pixel) over the layer's 4x4 output tiles"""
    d = (got.reshape(ref.shape).double() - ref.double()).abs()
    bar = 5e-5 * max(1.0, float(ref.abs().max()))
    c, y, x = np.unravel_index(int(d.argmax()), d.shape)
    ht = ref.shape[-1] // 4
    print("%s layer %d %s: max abs diff %.3g (|ref|max %.3g, bar %.3g) at channel %d pixel (%d, %d)" % (what, layer, tuple(ref.shape), float(d.max()), float(ref.abs().max()), bar, c, y, x))
    assert float(d.max()) < bar, "%s layer %d: %.3g at tile block %d, channel block %d (channel %d, pixel (%d, %d))" % (
        what, layer, float(d.max()), ((y // 4) * ht + x // 4) // 16, c // 16, c, y, x)


@pytest.mark.parametrize("state", ["synthetic", "seeded"])
def test_derived_u_is_bitwise_the_mirror(amd, probes, state):
    from affnet_amd import engine
    from affnet_amd._lib import ptr, check
    sd = _state(state)
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    want = wn.f43_packed_weight_transform(sd)
    for layer in (1, 3):
        w = want[layer].numpy()
        out = torch.zeros(w.size, device=DEV)
        check(probes.affnet_probe_hardnet_f43_u(ctx, ptr(packed), layer, ptr(out), None), ctx, "probe_hardnet_f43_u")
        torch.cuda.synchronize()
        bad = int((out.cpu().numpy().view(np.uint32) != w.view(np.uint32)).sum())
        print("%s conv%d: %d of %d derived U values differ from the mirror" % (state, layer, bad, w.size))
        assert bad == 0


def test_layers_1_and_3_against_torch(amd, probes):
    sd = _seeded_state(7)
    p = _patch()
    want = _torch_layers(sd, p)
    for layer in (1, 3):
        _check_layer(_dump(amd, probes, sd, p, layer, want[layer].numel()), want[layer], layer, "seeded state")


@pytest.mark.parametrize("layer", [1, 3])
def test_single_tap_weights(amd, probes, layer):
    base = _seeded_state(9)
    p = _patch()
    key = "features.%d.weight" % orc._TRUNK[layer][0]
    for tap in range(9):
        sd = {k: v.clone() for k, v in base.items()}
        w = torch.zeros_like(sd[key])
        w[:, :, tap // 3, tap % 3] = base[key][:, :, tap // 3, tap % 3]
        sd[key] = w
        want = _torch_layers(sd, p)[layer]
        _check_layer(_dump(amd, probes, sd, p, layer, want.numel()), want, layer, "tap (ky %d, kx %d)" % (tap // 3, tap % 3))


def test_outermost_ring_patch(amd, probes):
    sd = _seeded_state(7)
    p = _ring_patch()
    want = _torch_layers(sd, p)
    for layer in (1, 3):
        _check_layer(_dump(amd, probes, sd, p, layer, want[layer].numel()), want[layer], layer, "ring patch")


@pytest.fixture(scope="module")
def fixture_run(amd, probes):
    sd = orc.synthetic_hardnet_state(0)
    p = hardnet_fixture_batch()
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    return sd, p, packed, _forward(probes, packed, p.to(DEV)).clone()


@pytest.fixture(scope="module")
def fp64_bar(fixture_run):
    """(float64 descriptors of the fixture batch, bar): the bar is 2 x the CPU mirror's own max error on that batch - the factor covers the mirror's einsum
    contraction order, which is not the MFMA's k order (the direct form's mirror / GPU figures differ by about 1.3x) - and never above MODE_BAR"""
    sd, p, _, _ = fixture_run
    with torch.no_grad():
        want = orc.hardnet_forward({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, p.double())
        mirror = float((wn.hardnet_forward(sd, p, wino=True, poly=True, f43=wn.F43_LAYERS).double() - want).abs().max())
    return want, min(2.0 * mirror, MODE_BAR), mirror


def test_fixture_batch_against_fp64(fixture_run, fp64_bar):
    _, p, _, got = fixture_run
    want, bar, mirror = fp64_bar
    d = float((got.double().cpu() - want).abs().max())
    print("n = %d: max |form 2 descriptor - fp64| = %.3g; CPU mirror %.3g, bar %.3g" % (p.shape[0], d, mirror, bar))
    assert got.shape == (p.shape[0], 128) and d < bar, (d, bar)


def test_fused_descriptors_of_form_2_against_form_0(amd, weights, fp64_bar):
    A = amd.AffNetFast(PS=32); A.load_state_dict(weights["AffNet"]); A = A.to(DEV)
    O = amd.OriNetFast(PS=32); O.load_state_dict(weights["OriNet"]); O = O.to(DEV)
    H = _net(amd, weights["HardNet"])
    x = orc.synthetic_image(240, 320, 1).to(DEV)
    out = {}
    for form in (0, FORM):
        det = amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=300, border=5, num_Baum_iters=1, AffNet=A, OriNet=O).to(DEV)
        det.desc_form = form
        r = det.enqueue(x, do_ori=True, desc=H)
        torch.cuda.synchronize()
        out[form] = {k: r[k].clone() for k in ("count", "ids", "responses", "LAFs", "descriptors")}
    assert int(out[0]["count"][0]) == 300
    for k in ("count", "ids", "responses", "LAFs"):
        assert torch.equal(out[0][k], out[FORM][k]), k
    d = float((out[FORM]["descriptors"].double() - out[0]["descriptors"].double()).abs().max())
    bar = 1e-6 + fp64_bar[1]          # form 0 is within 1e-6 of float64, form 2 within the float64 bar
    print("fused descriptors, 300 keypoints at 320x240: max |form 2 - form 0| = %.3g (bar %.3g)" % (d, bar))
    assert not torch.equal(out[0]["descriptors"], out[FORM]["descriptors"]), "form 2 did not run another kernel"
    assert d < bar


def test_batch_splits_and_a_second_run_give_the_same_bits(probes, fixture_run):
    _, p, packed, whole = fixture_run
    pd = p.to(DEV)
    again = _forward(probes, packed, pd)
    assert torch.equal(whole, again), "a second run changed the descriptors"
    at = 0
    for n in (1, 2, 17):
        part = _forward(probes, packed, pd[at:at + n])
        assert torch.equal(part, whole[at:at + n]), "batch of %d" % n
        at += n


def test_blob_rewritten_in_place_is_used_by_the_next_call(amd, probes):
    dev = torch.device(DEV)
    p = hardnet_fixture_batch()[:17].to(DEV)
    H1, H2 = _net(amd, orc.synthetic_hardnet_state(0)), _net(amd, _seeded_state(13))
    first = _forward(probes, H1.packed_weights(dev), p).clone()
    want = _forward(probes, H2.packed_weights(dev), p).clone()
    assert not torch.equal(first, want)
    H1.packed_weights(dev).copy_(H2.packed_weights(dev))                          # same device buffer, new weights
    assert torch.equal(_forward(probes, H1.packed_weights(dev), p), want)


def test_blob_rewritten_in_place_is_used_by_a_graph_replay(amd, weights):
    dev = torch.device(DEV)
    A = amd.AffNetFast(PS=32); A.load_state_dict(weights["AffNet"]); A = A.to(DEV)
    O = amd.OriNetFast(PS=32); O.load_state_dict(weights["OriNet"]); O = O.to(DEV)
    H1, H2 = _net(amd, orc.synthetic_hardnet_state(0)), _net(amd, _seeded_state(13))
    x = orc.synthetic_image(240, 320, 1).to(DEV)

    def mk():
        det = amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=300, border=5, num_Baum_iters=1, AffNet=A, OriNet=O).to(DEV)
        det.desc_form = FORM
        return det

    want1 = mk().run(x, do_ori=True, desc=H1)
    want2 = mk().run(x, do_ori=True, desc=H2)
    assert torch.equal(want1["LAFs"], want2["LAFs"]) and not torch.equal(want1["descriptors"], want2["descriptors"])
    cap = mk().capture(x, do_ori=True, desc=H1)
    got1 = cap.run(x)
    for k in ("LAFs", "responses", "descriptors", "ids"):
        assert torch.equal(got1[k], want1[k]), k
    H1.packed_weights(dev).copy_(H2.packed_weights(dev))                          # the graph holds this address
    got2 = cap.run(x, check_weights=False)
    for k in ("LAFs", "responses", "descriptors", "ids"):
        assert torch.equal(got2[k], want2[k]), k
