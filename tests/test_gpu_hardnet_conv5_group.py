"""Descriptor form 3: the exact HardNet trunk of form 2 cut behind conv4 (cnn32_trunk_kernel<HardNet, 8, *, 6> stores conv4's tensor into the patch's 32 KB slot) and
conv5 as Winograd F(4x4, 3x3) for four patches per workgroup, in place in those slots (affnet_amd/csrc/hardnet_conv5_f43.hip: hardnet_conv5_f43_kernel).  Pinned here: the
derived U of layer 5 bit for bit; the conv5 kernel alone against a float64 torch layer on conv4 tensors taken from the form 3 trunk, at every tail-group size and a
full-plus-partial launch, with the nine single-tap weight states and on tensors whose live pixels are the outermost ring; that a patch's output does not depend on its group
or its neighbours; the fused descriptors of form 3 against form 2 (everything but the descriptors bit-equal); the descriptors against float64 on the ragged fixture batch at a
bar taken from the CPU mirror's own error; graph replay against eager; and that a blob rewritten in place never meets stale U - eagerly or in a replayed graph.
The patch-tensor calls go through libaffnet_hip_probes.so (affnet_probe_hardnet_c5_*): HardNet.forward always runs form 0."""
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
FORM = 3
COUNTS = (1, 2, 3, 4, 5, 17)    # every size of the last group (1, 2, 3, full) and launches of one full group + 1 and four full groups + 1


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
    for name in ("affnet_probe_hardnet_c5_trunk_layer", "affnet_probe_hardnet_c5_forward", "affnet_probe_hardnet_c5_layer", "affnet_probe_hardnet_c5_u"):
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


def _ctx():
    from affnet_amd import engine
    return engine.utility_ctx(torch.device(DEV))


def _conv5(probes, packed, x4):
    """The conv5 kernel alone: x4 (n, 128, 8, 8) post-ReLU conv4 tensors -> (n, 128, 8, 8) post-ReLU conv5 tensors, through the kernel's slot layouts"""
    from affnet_amd._lib import ptr, check
    n = x4.shape[0]
    slots = x4.to(DEV).float().reshape(n, 32, 4, 64).permute(0, 1, 3, 2).contiguous().reshape(n, 8192)       # [c / 4][pixel][c % 4]
    ctx = _ctx()
    check(probes.affnet_probe_hardnet_c5_layer(ctx, ptr(packed), ptr(slots), n, None), ctx, "probe_hardnet_c5_layer")
    torch.cuda.synchronize()
    return slots.reshape(n, 64, 128).permute(0, 2, 1).reshape(n, 128, 8, 8).cpu()                            # [pixel][channel]


def _layer5_fp64(sd, x4):
    ci, bi, _ = orc._TRUNK[5]
    with torch.no_grad():
        y = F.conv2d(x4.double(), sd["features.%d.weight" % ci].double(), None, padding=1)
        return F.relu(F.batch_norm(y, sd["features.%d.running_mean" % bi].double(), sd["features.%d.running_var" % bi].double(), None, None, False, 0.1, 1e-5))


def _check_layer(got, ref, what):
    """the project's layer bar; names the worst (patch, group column, channel block, pixel)"""
    d = (got.double() - ref).abs()
    bar = 5e-5 * max(1.0, float(ref.abs().max()))
    i, c, y, x = np.unravel_index(int(d.argmax()), d.shape)
    print("%s, n = %d: max abs diff %.3g (|ref|max %.3g, bar %.3g) at patch %d channel %d pixel (%d, %d)" % (what, ref.shape[0], float(d.max()), float(ref.abs().max()), bar, i, c, y, x))
    assert float(d.max()) < bar, "%s: %.3g at patch %d (column block %d of its group), channel block %d, tile (%d, %d)" % (what, float(d.max()), i, i % 4, c // 16, y // 4, x // 4)


@pytest.fixture(scope="module")
def conv4_run(amd, probes):
    """(state, packed blob, conv4 tensors (17, 128, 8, 8)) of 17 seeded patches, each dumped from the form 3 trunk's layer 4; computed once, never modified"""
    from affnet_amd._lib import ptr, check
    sd = _seeded_state(7)
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    p = (torch.rand(17, 32, 32, generator=torch.Generator().manual_seed(5)) * 255).to(DEV)
    ctx = _ctx()
    out = torch.zeros(17, 128 * 64, device=DEV)
    for i in range(17):
        check(probes.affnet_probe_hardnet_c5_trunk_layer(ctx, ptr(packed), ptr(p[i].contiguous()), 4, ptr(out[i]), None), ctx, "probe_hardnet_c5_trunk_layer")
    torch.cuda.synchronize()
    x4 = out.reshape(17, 128, 8, 8).cpu()
    assert float(x4.abs().max()) > 0 and bool((x4 >= 0).all())
    return sd, packed, x4


@pytest.mark.parametrize("state", ["synthetic", "seeded"])
def test_derived_u_is_bitwise_the_mirror(amd, probes, state):
    from affnet_amd._lib import ptr, check
    sd = _state(state)
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    ctx = _ctx()
    w = wn.f43_conv5_packed_weight_transform(sd).numpy()
    out = torch.zeros(w.size, device=DEV)
    check(probes.affnet_probe_hardnet_c5_u(ctx, ptr(packed), ptr(out), None), ctx, "probe_hardnet_c5_u")
    torch.cuda.synchronize()
    bad = int((out.cpu().numpy().view(np.uint32) != w.view(np.uint32)).sum())
    print("%s conv5: %d of %d derived U values differ from the mirror" % (state, bad, w.size))
    assert w.size == 36 * 128 * 128 and bad == 0


@pytest.mark.parametrize("n", COUNTS)
def test_layer_5_against_torch(probes, conv4_run, n):
    sd, packed, x4 = conv4_run
    _check_layer(_conv5(probes, packed, x4[:n]), _layer5_fp64(sd, x4[:n]), "seeded state")


def test_single_tap_weights(amd, probes, conv4_run):
    base, _, x4 = conv4_run
    key = "features.%d.weight" % orc._TRUNK[5][0]
    for tap in range(9):
        sd = {k: v.clone() for k, v in base.items()}
        w = torch.zeros_like(sd[key])
        w[:, :, tap // 3, tap % 3] = base[key][:, :, tap // 3, tap % 3]
        sd[key] = w
        packed = _net(amd, sd).packed_weights(torch.device(DEV))
        _check_layer(_conv5(probes, packed, x4[:5]), _layer5_fp64(sd, x4[:5]), "tap (ky %d, kx %d)" % (tap // 3, tap % 3))


def test_outermost_ring_only(probes, conv4_run):
    """only the outermost ring of the 8 x 8 tensor is live: what the edge tiles read next to their halo; alone and in a group beside full tensors"""
    sd, packed, x4 = conv4_run
    ring = torch.zeros_like(x4[:5])
    for sl in ((slice(0, 1), slice(None)), (slice(7, 8), slice(None)), (slice(None), slice(0, 1)), (slice(None), slice(7, 8))):
        ring[(slice(None), slice(None)) + sl] = x4[:5][(slice(None), slice(None)) + sl]
    _check_layer(_conv5(probes, packed, ring[:1]), _layer5_fp64(sd, ring[:1]), "ring tensor alone")
    mixed = torch.cat([x4[5:7], ring[2:3], x4[7:9]])
    _check_layer(_conv5(probes, packed, mixed), _layer5_fp64(sd, mixed), "ring tensor in column 2 of a full group")


def test_a_patch_does_not_depend_on_its_group(probes, conv4_run):
    _, packed, x4 = conv4_run
    whole = _conv5(probes, packed, x4)
    assert torch.equal(whole, _conv5(probes, packed, x4)), "a second run changed the layer"
    one = x4[3:4]
    alone = _conv5(probes, packed, one)
    assert torch.equal(alone[0], whole[3]), "alone against column 3 of group 0"
    first = _conv5(probes, packed, torch.cat([one, x4[9:16]]))
    assert torch.equal(first[0], alone[0]), "first of its batch"
    last = _conv5(probes, packed, torch.cat([x4[9:14], one]))             # 6 tensors: column 1 of a tail group of two
    assert torch.equal(last[5], alone[0]), "last of its batch"
    perm = torch.randperm(17, generator=torch.Generator().manual_seed(3))
    got = _conv5(probes, packed, x4[perm])
    assert torch.equal(got, whole[perm]), "permuted batch of 17"


def _forward(probes, packed, p):
    """Descriptors of form 3 for (n, 1, 32, 32) patches on the device, through the probe launch"""
    from affnet_amd._lib import ptr, check
    ctx = _ctx()
    n = p.shape[0]
    x = p[:, 0].contiguous().float()
    out = torch.empty(n, 128, device=DEV)
    scratch = torch.empty(n * (8192 + 512), device=DEV)
    check(probes.affnet_probe_hardnet_c5_forward(ctx, ptr(packed), ptr(x), n, ptr(out), ptr(scratch), None), ctx, "probe_hardnet_c5_forward")
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def fixture_run(amd, probes):
    sd = orc.synthetic_hardnet_state(0)
    p = hardnet_fixture_batch()
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    return sd, p, packed, _forward(probes, packed, p.to(DEV)).clone()


@pytest.fixture(scope="module")
def fp64_bar(fixture_run):
    """(float64 descriptors of the fixture batch, bar, mirror): the bar is 2 x the CPU mirror's own max error on that batch - the factor covers the mirror's einsum
    contraction order, which is not the MFMA's k order - and never above MODE_BAR: the rule of tests/test_gpu_hardnet_f43.py.  On the 301-patch fixture batch the
    mirror of form 3 is about 7e-7 from float64 (form 2: about 5e-7), so the bar is about 1.4e-6; the test prints the values it used."""
    sd, p, _, _ = fixture_run
    with torch.no_grad():
        want = orc.hardnet_forward({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, p.double())
        mirror = float((wn.hardnet_forward(sd, p, wino=True, poly=True, f43=wn.F43_LAYERS_FORM3).double() - want).abs().max())
    return want, min(2.0 * mirror, MODE_BAR), mirror


def test_fixture_batch_against_fp64(fixture_run, fp64_bar):
    _, p, _, got = fixture_run
    want, bar, mirror = fp64_bar
    d = float((got.double().cpu() - want).abs().max())
    print("n = %d: max |form 3 descriptor - fp64| = %.3g; CPU mirror %.3g, bar %.3g" % (p.shape[0], d, mirror, bar))
    assert got.shape == (p.shape[0], 128) and p.shape[0] == 301 and d < bar, (d, bar)


def _nets(amd, weights):
    A = amd.AffNetFast(PS=32); A.load_state_dict(weights["AffNet"]); A = A.to(DEV)
    O = amd.OriNetFast(PS=32); O.load_state_dict(weights["OriNet"]); O = O.to(DEV)
    return A, O


def _det(amd, A, O, form):
    det = amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=300, border=5, num_Baum_iters=1, AffNet=A, OriNet=O).to(DEV)
    det.desc_form = form
    return det


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fused_descriptors_of_form_3_against_form_2(amd, weights, fp64_bar, seed):
    A, O = _nets(amd, weights)
    H = _net(amd, weights["HardNet"])
    x = orc.synthetic_image(240, 320, seed).to(DEV)
    out = {}
    for form in (2, FORM):
        r = _det(amd, A, O, form).enqueue(x, do_ori=True, desc=H)
        torch.cuda.synchronize()
        out[form] = {k: r[k].clone() for k in ("count", "ids", "responses", "LAFs", "descriptors")}
    for k in ("count", "ids", "responses", "LAFs"):
        assert torch.equal(out[2][k], out[FORM][k]), k
    d = float((out[FORM]["descriptors"].double() - out[2]["descriptors"].double()).abs().max())
    bar = fp64_bar[1]                 # 2 x the CPU mirror's own distance from float64 (about 1.4e-6, see fp64_bar)
    print("fused descriptors, seed %d, %d keypoints at 320x240: max |form 3 - form 2| = %.3g (bar %.3g)" % (seed, int(out[2]["count"][0]), d, bar))
    assert int(out[2]["count"][0]) > 0
    assert not torch.equal(out[2]["descriptors"], out[FORM]["descriptors"]), "form 3 did not run another kernel"
    assert d < bar


def test_blob_rewritten_in_place_is_used_by_the_next_call(amd, probes):
    dev = torch.device(DEV)
    p = hardnet_fixture_batch()[:17].to(DEV)
    H1, H2 = _net(amd, orc.synthetic_hardnet_state(0)), _net(amd, _seeded_state(13))
    first = _forward(probes, H1.packed_weights(dev), p).clone()
    want = _forward(probes, H2.packed_weights(dev), p).clone()
    assert not torch.equal(first, want)
    H1.packed_weights(dev).copy_(H2.packed_weights(dev))                          # same device buffer, new weights
    assert torch.equal(_forward(probes, H1.packed_weights(dev), p), want)


def test_graph_replay_equals_eager_and_follows_a_blob_rewritten_in_place(amd, weights):
    dev = torch.device(DEV)
    A, O = _nets(amd, weights)
    H1, H2 = _net(amd, orc.synthetic_hardnet_state(0)), _net(amd, _seeded_state(13))
    x = orc.synthetic_image(240, 320, 1).to(DEV)
    want1 = _det(amd, A, O, FORM).run(x, do_ori=True, desc=H1)
    want2 = _det(amd, A, O, FORM).run(x, do_ori=True, desc=H2)
    assert torch.equal(want1["LAFs"], want2["LAFs"]) and not torch.equal(want1["descriptors"], want2["descriptors"])
    cap = _det(amd, A, O, FORM).capture(x, do_ori=True, desc=H1)
    got1 = cap.run(x)
    for k in ("LAFs", "responses", "descriptors", "ids"):
        assert torch.equal(got1[k], want1[k]), k
    H1.packed_weights(dev).copy_(H2.packed_weights(dev))                          # the graph holds this address
    got2 = cap.run(x, check_weights=False)
    for k in ("LAFs", "responses", "descriptors", "ids"):
        assert torch.equal(got2[k], want2[k]), k
