"""The exact HardNet trunk runs conv1 and conv3 in the paired row form of Winograd F(2x2, 3x3) (affnet_amd/csrc/cnn_mfma.h:
conv3x3_wino_mfma_pair_rows): two channel blocks of one tile block share one window transform, a step covers one row of four transform
positions, and the next step's reads and transform sit between the current step's MFMAs.  The descriptors stay bit-equal to the recorded ones
(tests/test_gpu_winograd_packed.py is the referee); pinned here: layers 1 and 3 against a torch CPU forward for two sets of weights, with the
channel block named when one is off, and that a patch's descriptor depends neither on the batch it travels in nor on the run."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402
from make_golden_hardnet_desc import hardnet_fixture_batch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _hardnet(seed):
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    H = affnet_amd.HardNet(); H.load_state_dict(orc.synthetic_hardnet_state(seed))
    return H.to(DEV)


@pytest.mark.parametrize("seed", [0, 3])
def test_hardnet_winograd_layers_1_and_3(seed):
    """Bar: that of test_orinet_trunk_layer_by_layer, 5e-5 * max(1, |ref|max) over the whole tensor."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    sd = orc.synthetic_hardnet_state(seed)
    p = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(5)) * 255
    with torch.no_grad():                                                         # the reference trunk: conv, eval BatchNorm (affine=False), ReLU
        x = orc.input_norm(p)
        want = []
        for ci, bi, st in orc._TRUNK:
            x = F.conv2d(x, sd["features.%d.weight" % ci], None, stride=st, padding=1)
            x = F.relu(F.batch_norm(x, sd["features.%d.running_mean" % bi], sd["features.%d.running_var" % bi], None, None, False, 0.1, 1e-5))
            want.append(x)
    packed = _hardnet(seed).packed_weights(torch.device(DEV))
    ctx = engine.utility_ctx(torch.device(DEV))
    pd = p[0, 0].to(DEV).contiguous()
    for layer in (1, 3):
        ref = want[layer][0]
        out = torch.zeros(ref.numel(), device=DEV)
        check(lib.affnet_cnn32_debug_layer(ctx, 2, ptr(packed), ptr(pd), layer, ptr(out), None), ctx, "debug_layer")
        torch.cuda.synchronize()
        diff = (out.cpu().reshape(ref.shape).double() - ref.double()).abs()
        per_block = diff.reshape(ref.shape[0] // 16, -1).max(dim=1).values       # one figure per block of 16 output channels
        bar = 5e-5 * max(1.0, float(ref.abs().max()))
        print("HardNet(seed %d) layer %d %s: max abs diff %.3g (|ref|max %.3g, bar %.3g); per channel block: %s"
              % (seed, layer, tuple(ref.shape), float(diff.max()), float(ref.abs().max()), bar, " ".join("%.3g" % v for v in per_block.tolist())))
        assert float(diff.max()) < bar, "layer %d, channel blocks over the bar: %s" % (layer, [i for i, v in enumerate(per_block.tolist()) if v >= bar])


def test_batches_of_1_2_17_and_a_second_run_give_the_same_bits():
    H = _hardnet(0)
    p = hardnet_fixture_batch()[:40].to(DEV)
    whole = H(p).clone()
    again = H(p).clone()
    parts = [H(p[0:1]).clone(), H(p[1:3]).clone(), H(p[3:20]).clone()]
    torch.cuda.synchronize()
    assert torch.equal(whole, again), "a second run changed the descriptors"
    for (lo, hi), part in zip(((0, 1), (1, 3), (3, 20)), parts):
        assert torch.equal(part, whole[lo:hi]), "patches %d..%d alone differ from the same patches inside the batch of %d" % (lo, hi - 1, p.shape[0])
