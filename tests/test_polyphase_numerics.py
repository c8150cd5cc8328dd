"""CPU pins of the polyphase Winograd F(2x2, 2x2) arithmetic of HardNet's stride-2 layers conv2 / conv4 in descriptor form 1 (tools/winograd_numerics.py:
poly_weight_transform, poly_input_transform, poly_conv3x3_s2 mirror the operation order of affnet_amd/csrc/cnn_mfma.h: conv3x3_poly_mfma_rows and
weights_layout.h: poly_weight_transform): the algebra equals the direct stride-2 convolution in float64 - on random operands, tap by tap and on the padded
border - the fp32 descriptors stay within the bar of tests/test_gpu_winograd.py, and a transformed weight is a tap or a sum of two taps along each axis."""
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

BAR64 = 1e-12
SIZES = (8, 16)


def _operands(h, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 16, h, h, generator=g, dtype=torch.float64), torch.randn(16, 16, 3, 3, generator=g, dtype=torch.float64)


def _diff(x, w):
    want = F.conv2d(x, w, None, stride=2, padding=1)
    got = wn.poly_conv3x3_s2(x, w)
    assert got.shape == want.shape
    return float((got - want).abs().max())


@pytest.mark.parametrize("h", SIZES)
def test_polyphase_algebra_equals_direct_stride2_convolution_in_fp64(h):
    x, w = _operands(h, 3 + h)
    d = _diff(x, w)
    print("H = %d: max |polyphase - conv2d| = %.3g" % (h, d))
    assert d < BAR64


@pytest.mark.parametrize("h", SIZES)
def test_single_tap_weights(h):
    x, w = _operands(h, 40 + h)
    for ky in range(3):
        for kx in range(3):
            w1 = torch.zeros_like(w)
            w1[:, :, ky, kx] = w[:, :, ky, kx]
            d = _diff(x, w1)
            assert d < BAR64, "tap (ky %d, kx %d) at H = %d: %.3g - a wrong phase or window offset" % (ky, kx, h, d)


@pytest.mark.parametrize("h", SIZES)
def test_border_only_inputs(h):
    x, w = _operands(h, 70 + h)
    xb = torch.zeros_like(x)
    for sl in ((slice(None), slice(None), 0), (slice(None), slice(None), h - 1), (slice(None), slice(None), slice(None), 0), (slice(None), slice(None), slice(None), h - 1)):
        xb[sl] = x[sl]
    d = _diff(xb, w)
    assert d < BAR64, "border rows / columns at H = %d: %.3g - the padding" % (h, d)


def test_fp32_mirror_descriptors_within_the_gpu_bar():
    sd = orc.synthetic_hardnet_state(0)
    p = torch.rand(64, 1, 32, 32, generator=torch.Generator().manual_seed(0)) * 255
    with torch.no_grad():
        ref = orc.hardnet_forward({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, p.double())
        d = float((wn.hardnet_forward(sd, p, wino=True, poly=True).double() - ref).abs().max())
    print("max |fp32 mirror descriptor (Winograd + polyphase) - fp64| on 64 patches: %.3g" % d)
    assert d < 1e-6          # the bar of tests/test_gpu_winograd.py


def test_packed_weight_transform_is_tap_or_sum_of_two_taps():
    sd = orc.synthetic_hardnet_state(0)
    packed = wn.poly_packed_weight_transform(sd)
    for layer in (2, 4):
        g = wn.packed_taps(sd, layer).numpy()                          # [co][ci][3][3] fp32
        co, ci = g.shape[:2]
        ax = lambda a0, a1, a2: [a0, a0 + a2, a2, a1, a1]              # along one axis: (g0, g0 + g2, g2 | g1, g1), one fp32 sum
        t = [ax(g[:, :, ky, 0], g[:, :, ky, 1], g[:, :, ky, 2]) for ky in range(3)]      # x first: t[ky][ix]
        want = np.empty((25, ci // 16, 4, co, 4), np.float32)
        for ix in range(5):
            col = ax(t[0][ix], t[1][ix], t[2][ix])                     # then y: col[iy]
            for iy in range(5):
                u = col[iy]
                assert u.dtype == np.float32
                want[wn.poly_xi(iy, ix)] = u.reshape(co, ci // 16, 4, 4).transpose(1, 2, 0, 3)      # [ci / 16][(c / 4) % 4][co][c % 4]
        got = packed[layer].numpy()
        assert got.size == 25 * ci * co
        assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32)), layer
    assert [wn.poly_xi(iy, ix) for iy in range(5) for ix in range(5)] == [0, 1, 2, 9, 10, 3, 4, 5, 11, 12, 6, 7, 8, 13, 14, 15, 16, 17, 21, 22, 18, 19, 20, 23, 24]
