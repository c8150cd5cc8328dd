"""CPU pins of the polyphase Winograd F(2x2, 2x2) arithmetic of the stride-2 layers of the 16-channel trunks (AffNet shape form 2 and the exact OriNet trunk:
conv2 16 -> 32 @32x32 -> 16x16, conv4 32 -> 64 @16x16 -> 8x8), as tools/winograd_numerics.py: poly16_conv2 / poly16_conv4 mirror the operation order of
affnet_amd/csrc/cnn_mfma.h: conv3x3_poly16_mfma_rows and poly16_combine - conv4 with its two K groups folded separately and added as K group 0 + K group 1.
In float64 the mirrors equal F.conv2d(stride=2, padding=1) - on seeded weights, on the shipped checkpoints' folded taps, tap by tap and on the padded border.
In fp32 the layer error (against the float64 convolution) stays below twice the direct fp32 form's own error on the same inputs: the form has no constant but 1
and one more addition per axis."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import winograd_numerics as wn  # noqa: E402

BAR64 = 1e-11
SHAPES = {2: (16, 32, 32), 4: (32, 64, 16)}          # layer: (cin, cout, input height)
LAYERS = (2, 4)


def _operands(layer, seed, dtype=torch.float64, n=2):
    ci, co, h = SHAPES[layer]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, ci, h, h, generator=g, dtype=torch.float64).to(dtype), torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64).to(dtype)


def _diff(layer, x, w):
    want = F.conv2d(x, w, None, stride=2, padding=1)
    got = wn.poly16_conv(layer, x, w)
    assert got.shape == want.shape
    return float((got - want).abs().max())


@pytest.mark.parametrize("layer", LAYERS)
def test_mirror_equals_direct_stride2_convolution_in_fp64_on_seeded_weights(layer):
    d = _diff(layer, *_operands(layer, 3 + layer))
    print("layer %d: max |polyphase - conv2d| = %.3g" % (layer, d))
    assert d < BAR64


@pytest.mark.parametrize("net", ("AffNet", "OriNet"))
@pytest.mark.parametrize("layer", LAYERS)
def test_mirror_equals_direct_stride2_convolution_in_fp64_on_the_shipped_weights(weights, net, layer):
    w = wn.folded(weights[net], torch.float64)[layer][0]
    x, _ = _operands(layer, 11 + layer)
    assert tuple(w.shape[:2]) == (SHAPES[layer][1], SHAPES[layer][0])
    d = _diff(layer, x, w)
    print("%s layer %d: max |polyphase - conv2d| = %.3g" % (net, layer, d))
    assert d < BAR64


@pytest.mark.parametrize("layer", LAYERS)
def test_single_tap_weights(layer):
    x, w = _operands(layer, 40 + layer)
    for ky in range(3):
        for kx in range(3):
            w1 = torch.zeros_like(w)
            w1[:, :, ky, kx] = w[:, :, ky, kx]
            d = _diff(layer, x, w1)
            assert d < BAR64, "layer %d, tap (ky %d, kx %d): %.3g - a wrong phase or window offset" % (layer, ky, kx, d)


@pytest.mark.parametrize("layer", LAYERS)
def test_border_only_inputs(layer):
    x, w = _operands(layer, 70 + layer)
    h = x.shape[-1]
    for name, sl in (("first row", (slice(None), slice(None), 0)), ("last row", (slice(None), slice(None), h - 1)),
                     ("first column", (slice(None), slice(None), slice(None), 0)), ("last column", (slice(None), slice(None), slice(None), h - 1))):
        xb = torch.zeros_like(x)
        xb[sl] = x[sl]
        d = _diff(layer, xb, w)
        assert d < BAR64, "layer %d, %s only: %.3g - the padding" % (layer, name, d)


def _fp32_errors(layer, x64, w64):
    x, w = x64.float(), w64.float()
    ref = F.conv2d(x.double(), w.double(), None, stride=2, padding=1)       # the float64 convolution of the SAME fp32 operands
    direct = float((F.conv2d(x, w, None, stride=2, padding=1).double() - ref).abs().max())
    poly = float((wn.poly16_conv(layer, x, w).double() - ref).abs().max())
    return direct, poly


@pytest.mark.parametrize("layer", LAYERS)
def test_fp32_layer_error_below_twice_the_direct_forms_on_seeded_weights(layer):
    direct, poly = _fp32_errors(layer, *_operands(layer, 100 + layer, n=8))
    print("layer %d, seeded: max |fp32 - fp64| direct %.3g, polyphase %.3g (ratio %.2f)" % (layer, direct, poly, poly / direct))
    assert poly < 2 * direct


@pytest.mark.parametrize("net", ("AffNet", "OriNet"))
@pytest.mark.parametrize("layer", LAYERS)
def test_fp32_layer_error_below_twice_the_direct_forms_on_the_shipped_weights(weights, net, layer):
    # the layer's real input: the post-ReLU output of the layer before it, on seeded smooth patches
    sd = weights[net]
    with torch.no_grad():
        x = wn.trunk16_layers(sd, wn.smooth_patches(8, seed=5 + layer), (), torch.float64)[layer - 1]
    direct, poly = _fp32_errors(layer, x, wn.folded(sd, torch.float64)[layer][0])
    print("%s layer %d: max |fp32 - fp64| direct %.3g, polyphase %.3g (ratio %.2f)" % (net, layer, direct, poly, poly / direct))
    assert poly < 2 * direct


def test_conv4_mirror_adds_the_k_groups_partial_outputs():
    x, w = _operands(4, 9, torch.float32)
    want = wn.poly_conv3x3_s2(x[:, :16], w[:, :16]) + wn.poly_conv3x3_s2(x[:, 16:], w[:, 16:])
    assert torch.equal(wn.poly16_conv4(x, w), want)
    assert torch.equal(wn.poly16_conv2(x[:, :16], w[:32, :16]), wn.poly_conv3x3_s2(x[:, :16], w[:32, :16]))
