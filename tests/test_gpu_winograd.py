"""HardNet on the exact path runs conv1, conv3 and conv5 as Winograd F(2x2, 3x3) (affnet_amd/csrc/cnn_mfma.h:
conv3x3_wino_mfma_pair_rows for conv1 / conv3, conv3x3_wino_mfma_shared_v for conv5):
the descriptors against a float64 forward of the same network, on ragged batch sizes and on degenerate patches, and bit-equal from
run to run."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402

DEV = "cuda:0"
BAR = 1e-6          # fp32 Winograd vs float64: measured on the CPU emulation (tools/winograd_numerics.py) ~3e-7


@pytest.fixture(scope="module")
def hardnet():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    sd = affnet_amd.synthetic_hardnet_state(0)
    H = affnet_amd.HardNet(); H.load_state_dict(sd); H = H.to(DEV)
    sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    return H, sd64


def _check(H, sd64, p):
    got = H(p.to(DEV)).double().cpu()
    with torch.no_grad():
        want = orc.hardnet_forward(sd64, p.double())
    d = float((got - want).abs().max()) if p.shape[0] else 0.0
    print("n = %d: max |desc - fp64| = %.3g" % (p.shape[0], d))
    assert got.shape == (p.shape[0], 128)
    assert d < BAR, d
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 17, 257, 3000])
def test_winograd_hardnet_vs_fp64(hardnet, n):
    H, sd64 = hardnet
    g = torch.Generator().manual_seed(1000 + n)
    _check(H, sd64, torch.rand(n, 1, 32, 32, generator=g) * 255)


@pytest.mark.gpu
def test_winograd_hardnet_degenerate_patches(hardnet):
    H, sd64 = hardnet
    g = torch.Generator().manual_seed(7)
    half = torch.rand(1, 1, 32, 32, generator=g) * 255
    half[..., :, :16] = 0.0                         # left half zero: tiles of exact zeros next to live ones
    top = torch.rand(1, 1, 32, 32, generator=g) * 255
    top[..., :16, :] = 0.0
    const = torch.full((1, 1, 32, 32), 7.0)         # std = 0 -> normalised input 0 -> every activation is bias-driven
    _check(H, sd64, torch.cat([half, top, const]))


@pytest.mark.gpu
def test_winograd_hardnet_run_to_run_bit_equal(hardnet):
    H, _ = hardnet
    g = torch.Generator().manual_seed(11)
    p = (torch.rand(600, 1, 32, 32, generator=g) * 255).to(DEV)
    a = H(p)
    b = H(p)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
