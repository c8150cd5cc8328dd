"""The exact OriNet trunk runs conv1 and conv3 as Winograd F(2x2, 3x3) (affnet_amd/csrc/cnn_mfma.h: conv3x3_wino_mfma_rows); AffNet stays in the
direct form (the shape filter behind it turns on the last bits of its output).  The transformed weights U = G g G^T are not part of the packed blob:
a kernel of the library derives them from the blob's BN-folded taps in front of every OriNet trunk launch (affnet_amd/csrc/cnn_trunk_orinet.hip:
wino_derive_u_kernel) into a buffer the context owns; the debug accessor derives them for an AffNet blob as well (same shapes).  Pinned here: the
derived U bit for bit for both blobs, the OriNet trunk layer by layer (tests/test_gpu_parity.py covers AffNet and HardNet), that a blob rewritten in place can never meet stale U - eagerly or
in a replayed graph - and that two runs give the same bits."""
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


def _second_weights(sd, seed):
    """A second set of weights of the same shapes: every conv kernel perturbed by seeded noise of 10 % of its own spread"""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    for i in (0, 3, 6, 9, 12, 15):
        w = out["features.%d.weight" % i]
        out["features.%d.weight" % i] = w + 0.1 * w.std() * torch.randn(w.shape, generator=g)
    return out


@pytest.mark.parametrize("kind,name", [(0, "AffNet"), (1, "OriNet")])
def test_derived_u_is_bitwise_the_mirror(amd, weights, kind, name):
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    packed = _net(amd, kind, weights[name]).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    for layer in (1, 3):
        U = wn.weight_transform(wn.packed_taps(weights[name], layer))            # [4][4][co][ci]
        co, ci = U.shape[2:]
        want = U.reshape(16, co, ci // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1).numpy()   # [xi][ci / 16][(c / 4) % 4][co][c % 4]
        out = torch.zeros(want.size, device=DEV)
        check(lib.affnet_cnn32_debug_winograd_u(ctx, kind, ptr(packed), layer, ptr(out), None), ctx, "debug_winograd_u")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print("%s conv%d: %d of %d derived U values differ from the mirror" % (name, layer, bad, want.size))
        assert bad == 0


def test_orinet_trunk_layer_by_layer(amd, weights):
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    p = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(5)) * 255
    sd = weights["OriNet"]
    with torch.no_grad():                                                         # the reference trunk: conv, eval BatchNorm (affine=False), ReLU
        x = orc.input_norm(p)
        want = []
        for ci, bi, st in orc._TRUNK:
            x = F.conv2d(x, sd["features.%d.weight" % ci], None, stride=st, padding=1)
            x = F.relu(F.batch_norm(x, sd["features.%d.running_mean" % bi], sd["features.%d.running_var" % bi], None, None, False, 0.1, 1e-5))
            want.append(x)
    packed = _net(amd, 1, sd).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    pd = p[0, 0].to(DEV).contiguous()
    for layer in range(6):
        ref = want[layer][0]
        out = torch.zeros(ref.numel(), device=DEV)
        check(lib.affnet_cnn32_debug_layer(ctx, 1, ptr(packed), ptr(pd), layer, ptr(out), None), ctx, "debug_layer")
        torch.cuda.synchronize()
        d = float((out.cpu().reshape(ref.shape).double() - ref.double()).abs().max())
        print("OriNet trunk layer %d %s: max abs diff %.3g (|ref|max %.3g)" % (layer, tuple(ref.shape), d, float(ref.abs().max())))
        assert d < 5e-5 * max(1.0, float(ref.abs().max())), "layer %d" % layer


@pytest.mark.parametrize("kind,name", [(0, "AffNet"), (1, "OriNet")])
def test_blob_rewritten_in_place_is_used_by_the_next_call(amd, weights, kind, name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "cnn_random_patches.npz"))
    p = torch.from_numpy(g["patches"]).to(DEV)
    net = _net(amd, kind, weights[name])
    first = net(p).clone()
    other = _net(amd, kind, _second_weights(weights[name], 11 + kind))
    want = other(p).clone()
    assert not torch.equal(first, want)
    blob = net.packed_weights(torch.device(DEV))
    blob.copy_(other.packed_weights(torch.device(DEV)))                           # same device buffer, new weights
    got = net(p)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_blob_rewritten_in_place_is_used_by_a_graph_replay(amd, weights):
    dev = torch.device(DEV)
    H = amd.HardNet(); H.load_state_dict(orc.synthetic_hardnet_state(0)); H = H.to(DEV)
    x = orc.synthetic_image(240, 320, 1).to(DEV)
    mk = lambda A, O: amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=300, border=5, num_Baum_iters=1, AffNet=A, OriNet=O).to(DEV)
    A1, O1 = _net(amd, 0, weights["AffNet"]), _net(amd, 1, weights["OriNet"])
    A2, O2 = _net(amd, 0, _second_weights(weights["AffNet"], 21)), _net(amd, 1, _second_weights(weights["OriNet"], 22))
    want1 = mk(A1, O1).run(x, do_ori=True, desc=H)
    want2 = mk(A2, O2).run(x, do_ori=True, desc=H)
    assert want1["LAFs"].shape != want2["LAFs"].shape or not torch.equal(want1["LAFs"], want2["LAFs"])
    cap = mk(A1, O1).capture(x, do_ori=True, desc=H)
    got1 = cap.run(x)
    for k in ("LAFs", "responses", "descriptors", "ids"):
        assert torch.equal(got1[k], want1[k]), k
    A1.packed_weights(dev).copy_(A2.packed_weights(dev))                          # the graph holds these addresses
    O1.packed_weights(dev).copy_(O2.packed_weights(dev))
    got2 = cap.run(x, check_weights=False)
    for k in ("LAFs", "responses", "descriptors", "ids"):
        assert torch.equal(got2[k], want2[k]), k


@pytest.mark.parametrize("kind,name", [(0, "AffNet"), (1, "OriNet")])
def test_two_calls_are_bit_equal(amd, weights, kind, name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "cnn_random_patches.npz"))
    p = torch.from_numpy(g["patches"]).to(DEV)
    net = _net(amd, kind, weights[name])
    a = net(p).clone()
    b = net(p).clone()
    c = torch.cat([net(p[:5]), net(p[5:])])
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
