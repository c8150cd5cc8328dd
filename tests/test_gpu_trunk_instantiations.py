"""The 18 instantiations of cnn32_trunk_kernel (affnet_amd/csrc/cnn_trunk.h: 3 nets x 3 arithmetic modes x product / stamped) are built per net
(cnn_trunk_affnet.hip, cnn_trunk_orinet.hip, cnn_trunk_hardnet.hip) and reached by the host layer (cnn32.hip: trunk_launch) through a getter of another
translation unit.  The rest of the suite launches the 9 product ones and, through the layer dumps, the 3 exact stamped ones.  Here every net runs in
every mode through its product and its stamped instantiation: the stamped one adds only cycle-counter stores, so the two outputs are bit-equal,
and every flow writes stamp 0 at its top and stamp 11 behind its conv5 loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NETS = {"AffNet": lambda amd: amd.AffNetFast(PS=32), "OriNet": lambda amd: amd.OriNetFast(PS=32), "HardNet": lambda amd: amd.HardNet()}


@pytest.fixture(scope="module")
def patches():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return (torch.rand(3, 1, 32, 32, generator=torch.Generator().manual_seed(18)) * 255).to(DEV)


@pytest.mark.parametrize("arith", ["fp32", "fp32_split3", "fp32_split2h"])
@pytest.mark.parametrize("name", ["AffNet", "OriNet", "HardNet"])
def test_stamped_instantiation_computes_what_the_product_one_does(weights, patches, name, arith):
    import affnet_amd
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr
    net = NETS[name](affnet_amd)
    net.load_state_dict(weights[name])
    net = net.to(DEV)
    net.arith = arith
    ctx = engine.utility_ctx(torch.device(DEV), arith)
    plain = net(patches).clone()
    stamps = torch.zeros(3 * 8 * 32, dtype=torch.int64, device=DEV)
    try:
        assert lib.affnet_cnn32_debug_timing(ctx, ptr(stamps)) == 0
        stamped = net(patches).clone()
        torch.cuda.synchronize()
    finally:
        lib.affnet_cnn32_debug_timing(ctx, None)
    t = stamps.cpu().reshape(3, 8, 32)
    print("%s %s: max abs diff stamped - product %.3g; ticks stamp 0 -> 11 per (patch, wave): min %d max %d"
          % (name, arith, float((stamped - plain).abs().max()), int((t[:, :, 11] - t[:, :, 0]).min()), int((t[:, :, 11] - t[:, :, 0]).max())))
    assert torch.equal(stamped, plain)
    assert bool((t[:, :, 0] != 0).all()) and bool((t[:, :, 11] != 0).all())
    assert bool((t[:, :, 11] > t[:, :, 0]).all())
