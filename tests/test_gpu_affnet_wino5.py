"""conv5 of AffNet's Winograd trunk (shape form 1, cnn32_trunk_kernel<AFFNET, 8, *, 1>) runs as F(2x2, 3x3) like OriNet's (affnet_amd/csrc/cnn_mfma.h:
conv3x3_wino_mfma_half_rows, wino5_combine), and the head reduces straight from the combined fragments (cnn_trunk.h: head_partials_wino).  Pinned here: the
derived U of layer 5 of an AffNet blob bit for bit against the mirror (tools/winograd_numerics.py), layer 5 of THIS kernel against a torch CPU forward with the
channel block and the position half named when one is off (libaffnet_hip_probes.so: affnet_probe_affnet_wino_layer; affnet_cnn32_debug_layer answers with the direct
trunk), and layer 4 bit for bit against the dump of the kernel before conv5 moved.  What the head does with the fragments is pinned by
tests/test_gpu_shape_form.py (|dA| of every unflagged candidate, batch split, graph replay).

tests/golden/affnet_wino_layer4_seed5.npy: layer 4 ([64][8][8] fp32) of the patch `torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(5)) * 255`
with the shipped AffNet weights, dumped on an MI355X by the library built from the commit in front of this change (Winograd conv1 / conv3, direct conv5) through the
same probe entry added to that build's probe library; the kernel's code up to layer 4 did not take part in the change."""
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
import affnet_oracle as orc  # noqa: E402
import winograd_numerics as wn  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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
    pl.affnet_probe_affnet_wino_layer.restype, pl.affnet_probe_affnet_wino_layer.argtypes = _lib.PROBE_SYMBOLS["affnet_probe_affnet_wino_layer"]
    return pl


def _net(amd, sd):
    net = amd.AffNetFast(PS=32)
    net.load_state_dict(sd)
    return net.to(DEV)


def _random_state(sd, seed):
    """Seeded random weights and BatchNorm statistics of AffNet's shapes (no dead channels, which could hide a wrong channel block)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if not torch.is_floating_point(v):
            out[k] = v.clone()
        elif k.endswith("running_var"):
            out[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("weight") and v.dim() == 4:
            out[k] = torch.randn(v.shape, generator=g) / float(v[0].numel()) ** 0.5
        else:
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
    return out


def _state(weights, state):
    return weights["AffNet"] if state == "shipped" else _random_state(weights["AffNet"], 7)


def _patch():
    return torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(5)) * 255


def _torch_layers(sd, p):
    """The reference trunk on the CPU: conv, eval BatchNorm (affine=False), ReLU; the six layers' outputs"""
    outs = []
    with torch.no_grad():
        x = orc.input_norm(p)
        for ci, bi, st in orc._TRUNK:
            x = F.conv2d(x, sd["features.%d.weight" % ci], None, stride=st, padding=1)
            x = F.relu(F.batch_norm(x, sd["features.%d.running_mean" % bi], sd["features.%d.running_var" % bi], None, None, False, 0.1, 1e-5))
            outs.append(x[0])
    return outs


def _dump(amd, probes, sd, p, layer, numel):
    from affnet_amd import engine
    from affnet_amd._lib import ptr, check
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    out = torch.zeros(numel, device=DEV)
    check(probes.affnet_probe_affnet_wino_layer(ctx, 0, ptr(packed), ptr(p[0, 0].to(DEV).contiguous()), layer, ptr(out), None), ctx, "probe_affnet_wino_layer")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("state", ["shipped", "seeded"])
def test_derived_u_of_layer_5_is_bitwise_the_mirror(amd, weights, state):
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    sd = _state(weights, state)
    packed = _net(amd, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    U = wn.weight_transform(wn.packed_taps(sd, 5))                               # [4][4][co][ci]
    co, ci = U.shape[2:]
    want = U.reshape(16, co, ci // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1).numpy()   # [xi][ci / 16][(c / 4) % 4][co][c % 4]
    assert want.size == 16 * 64 * 64
    out = torch.zeros(want.size, device=DEV)
    check(lib.affnet_cnn32_debug_winograd_u(ctx, 0, ptr(packed), 5, ptr(out), None), ctx, "debug_winograd_u")
    torch.cuda.synchronize()
    bad = int((out.cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum())
    print("AffNet (%s) conv5: %d of %d derived U values differ from the mirror" % (state, bad, want.size))
    assert bad == 0


@pytest.mark.parametrize("state", ["shipped", "seeded"])
def test_layer_5_of_the_winograd_kernel_against_torch(amd, probes, weights, state):
    """Bar: that of test_cnn_trunk_layer_by_layer, 5e-5 * max(1, |ref|max) over the whole tensor."""
    sd, p = _state(weights, state), _patch()
    ref = _torch_layers(sd, p)[5]                                                 # [64][8][8]
    out = _dump(amd, probes, sd, p, 5, ref.numel())
    diff = (out.reshape(ref.shape).double() - ref.double()).abs()
    # [channel block][16][tile row][position half = output row parity][8]: what one wave (2 * block + half) wrote
    per_wave = diff.reshape(4, 16, 4, 2, 8).permute(0, 3, 1, 2, 4).reshape(4, 2, -1).max(dim=2).values
    bar = 5e-5 * max(1.0, float(ref.abs().max()))
    print("AffNet (%s) Winograd kernel, layer 5: max abs diff %.3g (|ref|max %.3g, bar %.3g, %d of %d channels alive); per (channel block, position half): %s"
          % (state, float(diff.max()), float(ref.abs().max()), bar, int((ref.reshape(64, -1).abs().max(dim=1).values > 0).sum()), 64,
             " ".join("%.3g" % v for v in per_wave.reshape(-1).tolist())))
    over = [(cb, h) for cb in range(4) for h in range(2) if float(per_wave[cb, h]) >= bar]
    assert not over, "layer 5: (channel block, position half) over the bar: %s" % over


def test_layer_4_is_bitwise_the_recorded_parent(amd, probes, weights, golden_dir):
    """Nothing in front of conv5 moved: layer 4 of the fixed patch equals, bit for bit, the dump recorded from the kernel with the direct conv5 (see the head of this file)."""
    want = np.load(os.path.join(golden_dir, "affnet_wino_layer4_seed5.npy"))
    assert want.shape == (64, 8, 8) and want.dtype == np.float32
    got = _dump(amd, probes, weights["AffNet"], _patch(), 4, want.size).numpy().reshape(want.shape)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print("AffNet Winograd kernel, layer 4: %d of %d values differ from the recorded parent (max abs diff %.3g, |recorded|max %.3g)"
          % (bad, want.size, float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(want).max())))
    assert float(np.abs(want).max()) > 0
    assert bad == 0
