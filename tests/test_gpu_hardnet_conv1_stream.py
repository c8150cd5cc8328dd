"""Descriptor form 4: form 3 with conv0 + conv1 of the exact HardNet trunk streamed over conv1's K and conv1 as Winograd F(4x4, 3x3) (cnn32_trunk_kernel<HardNet, 8, *, 7>;
affnet_amd/csrc/cnn_trunk.h: the STREAM1 block, cnn_mfma.h: F43C1L).  Pinned here: the layer dump of conv1 against a float64 torch layer - on a seeded patch, with the nine
single-tap weight states, on patches whose only live pixels are one border row or column, and with weights that are live for ONE input channel of each quarter of each K
group - at 2 x the CPU mirror's own error on the same input; that a patch's descriptor does not depend on its batch or on the run; the fused descriptors of form 4
against form 3 (everything but the descriptors bit-equal); the descriptors against float64 on the ragged fixture batch at a bar taken from the CPU mirror's own error;
and graph replay against eager.  The patch-tensor calls go through libaffnet_hip_probes.so (affnet_probe_hardnet_c1_*): HardNet.forward always runs form 0.
conv1's derived U is pinned bit for bit by tests/test_gpu_hardnet_f43.py (affnet_probe_hardnet_f43_u, layer 1)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402
import winograd_numerics as wn  # noqa: E402
from make_golden_hardnet_desc import hardnet_fixture_batch  # noqa: E402
from test_winograd_f43_conv1_numerics import quarter_channel  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODE_BAR = 1e-5     # the project's HardNet bar between arithmetic modes (tests/test_gpu_parity.py): the float64 bar never exceeds it
FORM = 4
KEY1 = "features.%d.weight" % orc._TRUNK[1][0]


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
    for name in ("affnet_probe_hardnet_c1_trunk_layer", "affnet_probe_hardnet_c1_forward"):
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


def _ctx():
    from affnet_amd import engine
    return engine.utility_ctx(torch.device(DEV))


def _patch():
    return torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(5)) * 255


def _layer1(sd, p, dtype, f43):
    """post-ReLU output of layer 1 of the one patch: in float64 the reference; in float32 with f43 the CPU mirror of the kernel (conv0 direct, conv1 as f43_conv3x3)"""
    with torch.no_grad():
        x = orc.input_norm(p.to(dtype))
        layers = wn.folded(sd, dtype)
        w, b, st = layers[0]
        x = F.relu(F.conv2d(x, w, None, stride=st, padding=1) + b.view(1, -1, 1, 1))
        w, b, _ = layers[1]
        y = wn.f43_conv3x3(x, w) if f43 else F.conv2d(x, w, None, padding=1)
        return F.relu(y + b.view(1, -1, 1, 1))[0]


def _dump1(amd, probes, sd, p):
    from affnet_amd._lib import ptr, check
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    ctx = _ctx()
    out = torch.zeros(32 * 32 * 32, device=DEV)
    check(probes.affnet_probe_hardnet_c1_trunk_layer(ctx, ptr(packed), ptr(p[0, 0].to(DEV).contiguous()), 1, ptr(out), None), ctx, "probe_hardnet_c1_trunk_layer")
    torch.cuda.synchronize()
    return out.cpu().reshape(32, 32, 32)


def _check_layer1(amd, probes, sd, p, what):
    """bar = 2 x the CPU mirror's own error on the same input (the factor covers its contraction order: one matmul per position, not the MFMA's k order); names the
    worst (tile block, channel block, tile, pixel) of the layer's 4x4 output tiles"""
    ref = _layer1(sd, p, torch.float64, False)
    mirror = float((_layer1(sd, p, torch.float32, True).double() - ref).abs().max())
    d = (_dump1(amd, probes, sd, p).double() - ref).abs()
    bar = 2.0 * mirror
    c, y, x = np.unravel_index(int(d.argmax()), d.shape)
    print("%s: layer 1 max abs diff %.3g (|ref|max %.3g; CPU mirror %.3g, bar %.3g) at channel %d pixel (%d, %d)" % (what, float(d.max()), float(ref.abs().max()), mirror, bar, c, y, x))
    assert float(ref.abs().max()) > 0
    assert float(d.max()) < bar, "%s: %.3g (bar %.3g) at tile block %d, channel block %d, tile (%d, %d) (channel %d, pixel (%d, %d))" % (
        what, float(d.max()), bar, y // 8, c // 16, y // 4, x // 4, c, y, x)


def test_layer_1_against_torch(amd, probes):
    _check_layer1(amd, probes, _seeded_state(7), _patch(), "seeded state")


def test_single_tap_weights(amd, probes):
    base = _seeded_state(9)
    p = _patch()
    for tap in range(9):
        sd = {k: v.clone() for k, v in base.items()}
        w = torch.zeros_like(sd[KEY1])
        w[:, :, tap // 3, tap % 3] = base[KEY1][:, :, tap // 3, tap % 3]
        sd[KEY1] = w
        _check_layer1(amd, probes, sd, p, "tap (ky %d, kx %d)" % (tap // 3, tap % 3))


def test_border_only_patches(amd, probes):
    """only one border row or column of the patch is live: the windows that read the halo see the layer's largest steps"""
    sd = _seeded_state(7)
    full = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(6)) * 255
    for name, sl in (("row 0", (slice(0, 1), slice(None))), ("last row", (slice(31, 32), slice(None))), ("column 0", (slice(None), slice(0, 1))), ("last column", (slice(None), slice(31, 32)))):
        p = torch.zeros(1, 1, 32, 32)
        p[0, 0][sl] = full[0, 0][sl]
        _check_layer1(amd, probes, sd, p, "only %s live" % name)


def test_one_input_channel_per_quarter(amd, probes):
    """conv1's weights live for ONE input channel: one per quarter of each K group and its neighbour j (8 cases) - a wrong channel -> k-step map is a wrong layer"""
    base = _seeded_state(9)
    p = _patch()
    for G in range(2):
        for jh in range(2):
            for flip in range(2):
                c = quarter_channel(G, jh) ^ flip
                sd = {k: v.clone() for k, v in base.items()}
                w = torch.zeros_like(sd[KEY1])
                w[:, c] = base[KEY1][:, c]
                sd[KEY1] = w
                _check_layer1(amd, probes, sd, p, "input channel %d (K group %d, quarter %d)" % (c, G, jh))


def _forward(probes, packed, p):
    """Descriptors of form 4 for (n, 1, 32, 32) patches on the device, through the probe launch"""
    from affnet_amd._lib import ptr, check
    ctx = _ctx()
    n = p.shape[0]
    x = p[:, 0].contiguous().float()
    out = torch.empty(n, 128, device=DEV)
    scratch = torch.empty(n * (8192 + 512), device=DEV)
    check(probes.affnet_probe_hardnet_c1_forward(ctx, ptr(packed), ptr(x), n, ptr(out), ptr(scratch), None), ctx, "probe_hardnet_c1_forward")
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def fixture_run(amd, probes):
    sd = orc.synthetic_hardnet_state(0)
    p = hardnet_fixture_batch()
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    return sd, p, packed, _forward(probes, packed, p.to(DEV)).clone()


@pytest.fixture(scope="module")
def fp64_bars(fixture_run):
    """(float64 descriptors of the fixture batch, {form: bar}, {form: mirror}): a form's bar is 2 x the CPU mirror's own max error on that batch - the factor covers the
    mirror's einsum contraction order, which is not the MFMA's k order - and never above MODE_BAR: the rule of tests/test_gpu_hardnet_f43.py.  The test prints the values."""
    sd, p, _, _ = fixture_run
    with torch.no_grad():
        want = orc.hardnet_forward({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, p.double())
        mirror = {form: float((wn.hardnet_forward(sd, p, wino=True, poly=True, f43=layers).double() - want).abs().max())
                  for form, layers in ((3, wn.F43_LAYERS_FORM3), (4, wn.F43_LAYERS_FORM4))}
    return want, {form: min(2.0 * m, MODE_BAR) for form, m in mirror.items()}, mirror


def test_batches_of_1_2_17_and_a_second_run_give_the_same_bits(probes, fixture_run):
    """the workgroup is one patch: nothing may depend on a patch's neighbours (the conv5 kernel's groups of four are pinned by tests/test_gpu_hardnet_conv5_group.py)"""
    _, p, packed, whole = fixture_run
    x = p.to(DEV)
    got17 = _forward(probes, packed, x[:17])
    assert torch.equal(got17, whole[:17]), "17 patches against the first 17 of 301"
    assert torch.equal(_forward(probes, packed, x[:17]), got17), "a second run changed the descriptors"
    assert torch.equal(_forward(probes, packed, x[:1]), got17[:1]), "alone"
    assert torch.equal(_forward(probes, packed, x[:2]), got17[:2]), "a batch of two"


def test_fixture_batch_against_fp64(fixture_run, fp64_bars):
    _, p, _, got = fixture_run
    want, bars, mirror = fp64_bars
    d = float((got.double().cpu() - want).abs().max())
    print("n = %d: max |form 4 descriptor - fp64| = %.3g; CPU mirror %.3g, bar %.3g" % (p.shape[0], d, mirror[FORM], bars[FORM]))
    assert got.shape == (p.shape[0], 128) and p.shape[0] == 301 and d < bars[FORM], (d, bars[FORM])


def _nets(amd, weights):
    A = amd.AffNetFast(PS=32); A.load_state_dict(weights["AffNet"]); A = A.to(DEV)
    O = amd.OriNetFast(PS=32); O.load_state_dict(weights["OriNet"]); O = O.to(DEV)
    return A, O


def _det(amd, A, O, form):
    det = amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=300, border=5, num_Baum_iters=1, AffNet=A, OriNet=O).to(DEV)
    det.desc_form = form
    return det


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fused_descriptors_of_form_4_against_form_3(amd, weights, fp64_bars, seed):
    A, O = _nets(amd, weights)
    H = _net(amd, weights["HardNet"])
    x = orc.synthetic_image(240, 320, seed).to(DEV)
    out = {}
    for form in (3, FORM):
        r = _det(amd, A, O, form).enqueue(x, do_ori=True, desc=H)
        torch.cuda.synchronize()
        out[form] = {k: r[k].clone() for k in ("count", "ids", "responses", "LAFs", "descriptors")}
    for k in ("count", "ids", "responses", "LAFs"):
        assert torch.equal(out[3][k], out[FORM][k]), k
    d = float((out[FORM]["descriptors"].double() - out[3]["descriptors"].double()).abs().max())
    bar = fp64_bars[1][3] + fp64_bars[1][FORM]          # each form within its own float64 bar
    print("fused descriptors, seed %d, %d keypoints at 320x240: max |form 4 - form 3| = %.3g (bar %.3g = %.3g + %.3g)" % (seed, int(out[3]["count"][0]), d, bar, fp64_bars[1][3], fp64_bars[1][FORM]))
    assert int(out[3]["count"][0]) > 0
    assert not torch.equal(out[3]["descriptors"], out[FORM]["descriptors"]), "form 4 did not run another kernel"
    assert d < bar


def test_graph_replay_equals_eager(amd, weights):
    A, O = _nets(amd, weights)
    H = _net(amd, weights["HardNet"])
    x = orc.synthetic_image(240, 320, 1).to(DEV)
    want = _det(amd, A, O, FORM).run(x, do_ori=True, desc=H)
    cap = _det(amd, A, O, FORM).capture(x, do_ori=True, desc=H)
    for _ in range(2):
        got = cap.run(x)
        for k in ("LAFs", "responses", "descriptors", "ids"):
            assert torch.equal(got[k], want[k]), k
