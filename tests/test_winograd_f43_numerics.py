"""CPU pins of the Winograd F(4x4, 3x3) arithmetic of HardNet's descriptor form 2 (tools/winograd_numerics.py: f43_weight_transform, f43_input_transform,
f43_conv3x3 mirror the operation order of affnet_amd/csrc/cnn_mfma.h: f43_bt_lo / f43_bt_hi / f43_at_axis / f43_combine and weights_layout.h: f43_g_axis): the
algebra equals the direct convolution in float64 - on random operands at 32 x 32 and 16 x 16, tap by tap and on inputs whose only live pixels are one border row
or column - the transform matrices are the ones the mirror's sums spell out, the fp32 layer error stays below the project's layer bar and the fp32 descriptors
of form 2 below the bar the GPU test holds the kernel to."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402
import winograd_numerics as wn  # noqa: E402

BAR64 = 1e-11
SHAPES = ((32, 32), (16, 64))          # (H, channels) of conv1 and conv3

BT = [(4, 0, -5, 0, 1, 0), (0, -4, -4, 1, 1, 0), (0, 4, -4, -1, 1, 0), (0, -2, -1, 2, 1, 0), (0, 2, -1, -2, 1, 0), (0, 4, 0, -5, 0, 1)]
G = [(1 / 4, 0, 0), (-1 / 6, -1 / 6, -1 / 6), (-1 / 6, 1 / 6, -1 / 6), (1 / 24, 1 / 12, 1 / 6), (1 / 24, -1 / 12, 1 / 6), (0, 0, 1)]
AT = [(1, 1, 1, 1, 1, 0), (0, 1, -1, 2, -2, 0), (0, 1, 1, 4, 4, 0), (0, 1, -1, 8, -8, 1)]


def _operands(h, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, c, h, h, generator=g, dtype=torch.float64), torch.randn(c, c, 3, 3, generator=g, dtype=torch.float64) / (3.0 * c ** 0.5)


def _diff(x, w):
    want = F.conv2d(x, w, None, padding=1)
    got = wn.f43_conv3x3(x, w)
    assert got.shape == want.shape
    return float((got - want).abs().max())


def test_axis_sums_are_the_transform_matrices():
    """each axis function applied to the unit vectors gives the columns of B^T, G and A^T"""
    one = lambda n, k: [torch.tensor(1.0 if i == k else 0.0, dtype=torch.float64) for i in range(n)]
    for fn, mat, n in ((wn._f43_bt_axis, BT, 6), (wn._f43_g_axis, G, 3), (wn._f43_at_axis, AT, 6)):
        for k in range(n):
            col = [float(v) for v in fn(*one(n, k))]
            want = [float(row[k]) for row in mat]
            assert max(abs(a - b) for a, b in zip(col, want)) < 1e-15, (fn.__name__, k, col, want)


@pytest.mark.parametrize("h,c", SHAPES)
def test_f43_algebra_equals_direct_convolution_in_fp64(h, c):
    x, w = _operands(h, c, 3 + h)
    d = _diff(x, w)
    print("H = %d: max |F(4x4, 3x3) - conv2d| = %.3g" % (h, d))
    assert d < BAR64


@pytest.mark.parametrize("h,c", SHAPES)
def test_single_tap_weights(h, c):
    x, w = _operands(h, c, 40 + h)
    for ky in range(3):
        for kx in range(3):
            w1 = torch.zeros_like(w)
            w1[:, :, ky, kx] = w[:, :, ky, kx]
            d = _diff(x, w1)
            assert d < BAR64, "tap (ky %d, kx %d) at H = %d: %.3g - a wrong position or window offset" % (ky, kx, h, d)


@pytest.mark.parametrize("h,c", SHAPES)
def test_border_only_inputs(h, c):
    x, w = _operands(h, c, 70 + h)
    for name, sl in (("row 0", (slice(None), slice(None), 0)), ("last row", (slice(None), slice(None), h - 1)),
                     ("column 0", (slice(None), slice(None), slice(None), 0)), ("last column", (slice(None), slice(None), slice(None), h - 1))):
        xb = torch.zeros_like(x)
        xb[sl] = x[sl]
        d = _diff(xb, w)
        assert d < BAR64, "only %s live at H = %d: %.3g - the padding / the halo of the edge tiles" % (name, h, d)


@pytest.mark.parametrize("h,c", SHAPES)
def test_fp32_layer_error_within_the_layer_bar(h, c):
    x, w = _operands(h, c, 100 + h)
    ref = F.conv2d(x, w, None, padding=1)
    x32, w32 = x.float(), w.float()
    ref32 = F.conv2d(x32.double(), w32.double(), None, padding=1)           # the float64 result of the fp32 operands
    d = float((wn.f43_conv3x3(x32, w32).double() - ref32).abs().max())
    bar = 5e-5 * max(1.0, float(ref.abs().max()))
    print("H = %d: fp32 F(4x4, 3x3) layer error %.3g (|ref|max %.3g, bar %.3g)" % (h, d, float(ref.abs().max()), bar))
    assert d < bar


def test_fp32_mirror_descriptors_of_form_2():
    """the bar of tests/test_gpu_hardnet_f43.py is 2 x this mirror's error on its batch and never above 1e-5 (the project's HardNet bar between arithmetic modes)"""
    sd = orc.synthetic_hardnet_state(0)
    p = torch.rand(64, 1, 32, 32, generator=torch.Generator().manual_seed(0)) * 255
    with torch.no_grad():
        ref = orc.hardnet_forward({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, p.double())
        d1 = float((wn.hardnet_forward(sd, p, wino=True, poly=True).double() - ref).abs().max())
        d2 = float((wn.hardnet_forward(sd, p, wino=True, poly=True, f43=wn.F43_LAYERS).double() - ref).abs().max())
        d13 = float((wn.hardnet_forward(sd, p, wino=True, poly=True, f43=(1, 3)).double() - ref).abs().max())
    print("max |fp32 mirror descriptor - fp64| on 64 patches: form 1 %.3g, form 2 (conv3 in F(4x4, 3x3)) %.3g, conv1 and conv3 in F(4x4, 3x3) %.3g; GPU bar = 2 x "
          "the mirror's error, at most 1e-5" % (d1, d2, d13))
    assert 2.0 * d2 < 1e-5 and 2.0 * d13 < 1e-5
