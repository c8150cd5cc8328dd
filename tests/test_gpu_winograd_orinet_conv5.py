"""conv5 of the exact OriNet trunk runs as Winograd F(2x2, 3x3) too (affnet_amd/csrc/cnn_mfma.h: conv3x3_wino_mfma_half_rows, wino5_combine): the two waves
of a channel block take two of the four position rows each, exchange one row through LDS in a fixed order, and each writes one row of every 2 x 2-pixel tile into the
head's LDS copy.  Its U is derived with conv1's and conv3's in front of every launch.  Pinned here: the derived U of layer 5 bit for bit against the mirror
(tools/winograd_numerics.py), layer 5 against a torch CPU forward with the channel block and the position half named when one is off, that a patch's output
depends neither on the batch it travels in nor on the run, and that the fused pipeline and the stand-alone forward take the same loop."""
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


def _net(amd, kind, sd):
    net = (amd.AffNetFast if kind == 0 else amd.OriNetFast)(PS=32)
    net.load_state_dict(sd)
    return net.to(DEV)


def _random_state(sd, seed):
    """Seeded random weights and BatchNorm statistics of OriNet's shapes"""
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


@pytest.mark.parametrize("state", ["shipped", "seeded"])
def test_derived_u_of_layer_5_is_bitwise_the_mirror(amd, weights, state):
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    sd = weights["OriNet"] if state == "shipped" else _random_state(weights["OriNet"], 7)
    packed = _net(amd, 1, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    U = wn.weight_transform(wn.packed_taps(sd, 5))                               # [4][4][co][ci]
    co, ci = U.shape[2:]
    want = U.reshape(16, co, ci // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1).numpy()   # [xi][ci / 16][(c / 4) % 4][co][c % 4]
    assert want.size == 16 * 64 * 64
    out = torch.zeros(want.size, device=DEV)
    check(lib.affnet_cnn32_debug_winograd_u(ctx, 1, ptr(packed), 5, ptr(out), None), ctx, "debug_winograd_u")
    torch.cuda.synchronize()
    bad = int((out.cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum())
    print("OriNet (%s) conv5: %d of %d derived U values differ from the mirror" % (state, bad, want.size))
    assert bad == 0


def test_orinet_layer_5_against_torch(amd, weights):
    """Bar: that of test_orinet_trunk_layer_by_layer, 5e-5 * max(1, |ref|max) over the whole tensor."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    p = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(5)) * 255
    sd = weights["OriNet"]
    with torch.no_grad():                                                         # the reference trunk: conv, eval BatchNorm (affine=False), ReLU
        x = orc.input_norm(p)
        for ci, bi, st in orc._TRUNK:
            x = F.conv2d(x, sd["features.%d.weight" % ci], None, stride=st, padding=1)
            x = F.relu(F.batch_norm(x, sd["features.%d.running_mean" % bi], sd["features.%d.running_var" % bi], None, None, False, 0.1, 1e-5))
    ref = x[0]                                                                    # [64][8][8]
    packed = _net(amd, 1, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    out = torch.zeros(ref.numel(), device=DEV)
    check(lib.affnet_cnn32_debug_layer(ctx, 1, ptr(packed), ptr(p[0, 0].to(DEV).contiguous()), 5, ptr(out), None), ctx, "debug_layer")
    torch.cuda.synchronize()
    diff = (out.cpu().reshape(ref.shape).double() - ref.double()).abs()
    # [channel block][16][tile row][position half = output row parity][8]: what one wave (2 * block + half) wrote
    per_wave = diff.reshape(4, 16, 4, 2, 8).permute(0, 3, 1, 2, 4).reshape(4, 2, -1).max(dim=2).values
    bar = 5e-5 * max(1.0, float(ref.abs().max()))
    print("OriNet layer 5: max abs diff %.3g (|ref|max %.3g, bar %.3g); per (channel block, position half): %s"
          % (float(diff.max()), float(ref.abs().max()), bar, " ".join("%.3g" % v for v in per_wave.reshape(-1).tolist())))
    over = [(cb, h) for cb in range(4) for h in range(2) if float(per_wave[cb, h]) >= bar]
    assert not over, "layer 5: (channel block, position half) over the bar: %s" % over


def test_batches_of_1_2_17_and_a_second_run_give_the_same_bits(amd, weights):
    g = np.load(os.path.join(ROOT, "tests", "golden", "cnn_random_patches.npz"))
    p = torch.from_numpy(g["patches"])[:20].to(DEV)
    assert p.shape[0] == 20
    O = _net(amd, 1, weights["OriNet"])
    whole = O(p).clone()
    again = O(p).clone()
    parts = [O(p[0:1]).clone(), O(p[1:3]).clone(), O(p[3:20]).clone()]
    torch.cuda.synchronize()
    assert torch.equal(whole, again), "a second run changed the output"
    for (lo, hi), part in zip(((0, 1), (1, 3), (3, 20)), parts):
        assert torch.equal(part, whole[lo:hi]), "patches %d..%d alone differ from the same patches inside the batch of 20" % (lo, hi - 1)


def test_fused_pipeline_equals_staged_orinet(amd, weights):
    """The fused prologue (patches sampled inside the trunk kernel) and the stand-alone forward (patch tensors) run the same conv5 loop: bit-equal rows."""
    A, O = _net(amd, 0, weights["AffNet"]), _net(amd, 1, weights["OriNet"])
    x = orc.synthetic_image(240, 320, 1).to(DEV)

    class Foreign(torch.nn.Module):      # not a native net object -> forces the staged path
        def __init__(self, net):
            super().__init__()
            self.net, self.PS = net, 32

        def forward(self, patches, *a):
            return self.net(patches)

    mk = lambda ori: amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=300, border=5, num_Baum_iters=1, AffNet=A, OriNet=ori).to(DEV)
    fused, staged = mk(O), mk(Foreign(O))
    L1, r1 = fused(x, do_ori=True)
    L2, r2 = staged(x, do_ori=True)
    assert torch.equal(r1, r2) and torch.equal(fused.last_ids, staged.last_ids)
    assert torch.equal(L1, L2), "max LAF diff %g" % float((L1 - L2).abs().max())
