"""CPU pins of conv5 of HardNet's descriptor form 3 (tools/winograd_numerics.py: f43_conv5_grouped mirrors affnet_amd/csrc/hardnet_conv5_f43.hip: 128 -> 128 channels
at 8 x 8 as Winograd F(4x4, 3x3), the four 4x4 tiles of a patch): the algebra equals the direct convolution in float64 - on seeded operands and on the synthetic
HardNet state's layer 5, tap by tap and on inputs whose only live pixels are one border row or column - the fp32 layer error stays below the project's layer bar, and the
fp32 descriptors of form 3 stay below the bar the GPU test (tests/test_gpu_hardnet_conv5_group.py) holds the kernels to."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402
import winograd_numerics as wn  # noqa: E402

BAR64 = 1e-11          # the float64 leg of tests/test_winograd_f43_numerics.py
MODE_BAR = 1e-5        # the project's HardNet bar between arithmetic modes: no float64 bar exceeds it
N = 5                  # patches: one full group of four and a tail of one


def _operands(seed, n=N):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 128, 8, 8, generator=g, dtype=torch.float64), torch.randn(128, 128, 3, 3, generator=g, dtype=torch.float64) / (3.0 * 128 ** 0.5)


def _synthetic_layer5():
    """post-ReLU conv4 tensors of the synthetic HardNet state on seeded patches, and its BN-folded layer 5, in float64"""
    sd = orc.synthetic_hardnet_state(0)
    p = torch.rand(N, 1, 32, 32, generator=torch.Generator().manual_seed(11)) * 255
    with torch.no_grad():
        x = orc.input_norm(p.double())
        layers = wn.folded(sd, torch.float64)
        for w, b, st in layers[:5]:
            x = F.relu(F.conv2d(x, w, None, stride=st, padding=1) + b.view(1, -1, 1, 1))
    return x, layers[5][0]


def _diff(x, w):
    want = F.conv2d(x, w, None, padding=1)
    got = wn.f43_conv5_grouped(x, w)
    assert got.shape == want.shape
    return float((got - want).abs().max())


def test_algebra_equals_direct_convolution_in_fp64():
    d = _diff(*_operands(3))
    ds = _diff(*_synthetic_layer5())
    print("max |F(4x4, 3x3) conv5 - conv2d| in float64: seeded %.3g, synthetic state's layer 5 %.3g" % (d, ds))
    assert d < BAR64 and ds < BAR64


def test_single_tap_weights():
    x, w = _operands(40)
    for ky in range(3):
        for kx in range(3):
            w1 = torch.zeros_like(w)
            w1[:, :, ky, kx] = w[:, :, ky, kx]
            d = _diff(x, w1)
            assert d < BAR64, "tap (ky %d, kx %d): %.3g - a wrong position or window offset" % (ky, kx, d)


def test_border_only_inputs():
    x, w = _operands(70)
    for name, sl in (("row 0", (slice(None), slice(None), 0)), ("last row", (slice(None), slice(None), 7)),
                     ("column 0", (slice(None), slice(None), slice(None), 0)), ("last column", (slice(None), slice(None), slice(None), 7))):
        xb = torch.zeros_like(x)
        xb[sl] = x[sl]
        d = _diff(xb, w)
        assert d < BAR64, "only %s live: %.3g - the padding / the halo of the edge tiles" % (name, d)


def test_fp32_layer_error_within_the_layer_bar():
    for what, (x, w) in (("seeded", _operands(100)), ("synthetic layer 5", _synthetic_layer5())):
        ref = F.conv2d(x, w, None, padding=1)
        x32, w32 = x.float(), w.float()
        ref32 = F.conv2d(x32.double(), w32.double(), None, padding=1)           # the float64 result of the fp32 operands
        d = float((wn.f43_conv5_grouped(x32, w32).double() - ref32).abs().max())
        bar = 5e-5 * max(1.0, float(ref.abs().max()))
        print("%s: fp32 F(4x4, 3x3) conv5 layer error %.3g (|ref|max %.3g, bar %.3g)" % (what, d, float(ref.abs().max()), bar))
        assert d < bar


def test_fp32_mirror_descriptors_of_form_3():
    """the bar of tests/test_gpu_hardnet_conv5_group.py is 2 x this mirror's error on its batch and never above 1e-5, derived as tests/test_winograd_f43_numerics.py
    derives form 2's: the mirror's own distance from float64, the factor 2 for its contraction order (one matmul per position, not the MFMA's k order)"""
    sd = orc.synthetic_hardnet_state(0)
    p = torch.rand(64, 1, 32, 32, generator=torch.Generator().manual_seed(0)) * 255
    with torch.no_grad():
        ref = orc.hardnet_forward({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, p.double())
        d2 = float((wn.hardnet_forward(sd, p, wino=True, poly=True, f43=wn.F43_LAYERS).double() - ref).abs().max())
        d3 = float((wn.hardnet_forward(sd, p, wino=True, poly=True, f43=wn.F43_LAYERS_FORM3).double() - ref).abs().max())
    print("max |fp32 mirror descriptor - fp64| on 64 patches: form 2 %.3g, form 3 (conv5 in F(4x4, 3x3) as well) %.3g; GPU bar = 2 x the mirror's error = %.3g, at most %.0e"
          % (d2, d3, 2.0 * d3, MODE_BAR))
    assert 2.0 * d3 < MODE_BAR
