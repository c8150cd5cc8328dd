"""CPU pins of conv1 of HardNet's descriptor form 4 (affnet_amd/csrc/cnn_trunk.h: the STREAM1 block; cnn_mfma.h: F43C1L): 32 -> 32 channels at 32 x 32 as Winograd
F(4x4, 3x3), streamed with conv0 over its K - two K groups of 16 channels, each in two quarters of 8 (k-steps 2 jh, 2 jh + 1 = channels 16 G + 4 kq + 2 jh + {0, 1}).
tools/winograd_numerics.py: f43_conv3x3 is the mirror (every accumulator sums its own 32 products, lane-local transforms on both sides).  Pinned: the algebra equals the
direct convolution in float64 - on seeded operands and on the synthetic HardNet state's layer 1, tap by tap, on inputs whose only live pixels are one border row or
column (the windows that read the halo), and with weights that are live for ONE input channel of each quarter of each K group (a wrong channel -> k-step map is a wrong
layer, not noise); the fp32 layer error and the fp32 descriptors of form 4, from which tests/test_gpu_hardnet_conv1_stream.py takes its bars; and the LDS bank model of
the layer's three access patterns."""
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
N = 2


def quarter_channel(G, jh):
    """one input channel of quarter jh of K group G, another (kq, j) for every quarter: channel 16 G + 4 kq + 2 jh + j"""
    return 16 * G + 4 * ((2 * G + jh + 1) % 4) + 2 * jh + (G + jh) % 2


def _operands(seed, n=N):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 32, 32, 32, generator=g, dtype=torch.float64), torch.randn(32, 32, 3, 3, generator=g, dtype=torch.float64) / (3.0 * 32 ** 0.5)


def _synthetic_layer1():
    """post-ReLU conv0 tensors of the synthetic HardNet state on seeded patches, and its BN-folded layer 1, in float64"""
    sd = orc.synthetic_hardnet_state(0)
    p = torch.rand(N, 1, 32, 32, generator=torch.Generator().manual_seed(11)) * 255
    with torch.no_grad():
        x = orc.input_norm(p.double())
        layers = wn.folded(sd, torch.float64)
        w, b, st = layers[0]
        x = F.relu(F.conv2d(x, w, None, stride=st, padding=1) + b.view(1, -1, 1, 1))
    return x, layers[1][0]


def _diff(x, w):
    want = F.conv2d(x, w, None, padding=1)
    got = wn.f43_conv3x3(x, w)
    assert got.shape == want.shape
    return float((got - want).abs().max())


def test_algebra_equals_direct_convolution_in_fp64():
    d = _diff(*_operands(3))
    ds = _diff(*_synthetic_layer1())
    print("max |F(4x4, 3x3) conv1 - conv2d| in float64: seeded %.3g, synthetic state's layer 1 %.3g" % (d, ds))
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
    for name, sl in (("row 0", (slice(None), slice(None), 0)), ("last row", (slice(None), slice(None), 31)),
                     ("column 0", (slice(None), slice(None), slice(None), 0)), ("last column", (slice(None), slice(None), slice(None), 31))):
        xb = torch.zeros_like(x)
        xb[sl] = x[sl]
        d = _diff(xb, w)
        assert d < BAR64, "only %s live: %.3g - the padding / the halo of the edge tiles" % (name, d)


def test_one_input_channel_per_quarter():
    x, w = _operands(90)
    seen = set()
    for G in range(2):
        for jh in range(2):
            for flip in range(2):                       # both channels j of a (kq, quarter) over the eight cases
                c = quarter_channel(G, jh) ^ flip
                assert c // 16 == G and (c % 4) // 2 == jh and c not in seen
                seen.add(c)
                w1 = torch.zeros_like(w)
                w1[:, c] = w[:, c]
                d = _diff(x, w1)
                assert d < BAR64, "only input channel %d (K group %d, quarter %d) live: %.3g" % (c, G, jh, d)
    assert len(seen) == 8


def test_fp32_layer_error_is_recorded():
    """F(4x4, 3x3) at 32 channels costs about 18 x the F(2x2, 3x3) layer error (1.15e-4 against 6.5e-6 at |ref|max 23.0 on the synthetic state when this was written):
    recorded here, and held to 2 x that record relative to the layer's scale - not tighter, the mirror's own error is the yardstick"""
    for what, (x, w) in (("seeded", _operands(100)), ("synthetic layer 1", _synthetic_layer1())):
        x32, w32 = x.float(), w.float()
        ref32 = F.conv2d(x32.double(), w32.double(), None, padding=1)           # the float64 result of the fp32 operands
        d43 = float((wn.f43_conv3x3(x32, w32).double() - ref32).abs().max())
        d23 = float((wn.wino_conv3x3(x32, w32).double() - ref32).abs().max())
        bar = 2.0 * 1.15e-4 * max(1.0, float(ref32.abs().max())) / 23.0
        print("%s: fp32 conv1 layer error F(4x4, 3x3) %.3g, F(2x2, 3x3) %.3g (|ref|max %.3g, bar %.3g)" % (what, d43, d23, float(ref32.abs().max()), bar))
        assert d43 < bar


def test_fp32_mirror_descriptors_of_form_4():
    """the float64 bar of tests/test_gpu_hardnet_conv1_stream.py is 2 x this mirror's error on its batch and never above 1e-5, derived as the bars of forms 2 and 3 are:
    the mirror's own distance from float64, the factor 2 for its contraction order (one matmul per position, not the MFMA's k order)"""
    sd = orc.synthetic_hardnet_state(0)
    p = torch.rand(64, 1, 32, 32, generator=torch.Generator().manual_seed(0)) * 255
    with torch.no_grad():
        ref = orc.hardnet_forward({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, p.double())
        d3 = wn.hardnet_forward(sd, p, wino=True, poly=True, f43=wn.F43_LAYERS_FORM3).double()
        d4 = wn.hardnet_forward(sd, p, wino=True, poly=True, f43=wn.F43_LAYERS_FORM4).double()
    e3, e4, apart = float((d3 - ref).abs().max()), float((d4 - ref).abs().max()), float((d4 - d3).abs().max())
    print("max |fp32 mirror descriptor - fp64| on 64 patches: form 3 %.3g, form 4 (conv1 in F(4x4, 3x3) as well) %.3g, the two %.3g apart; GPU bar = 2 x the mirror's error = %.3g, at most %.0e"
          % (e3, e4, apart, 2.0 * e4, MODE_BAR))
    assert 2.0 * e4 < MODE_BAR


# ---- the layer's LDS access patterns against the bank rule of gfx950 -----------------------------------------------------------------------
# ds_read_b32 and every ds_write: bank = dword address mod 32, conflicts within each 32-lane half; ds_read_b64: mod 64, within each 32-lane half (8 bytes = 2 banks).
GS, WP, V, XS = 4676, 34, 4 * 4676, 512             # cnn_mfma.h: F43C1L


def _slot(kq, m):
    return 16 * kq + ((m + 4 * kq) & 15)


def _ways(addrs, banks, width=1):
    """the worst number of distinct addresses on one bank over the two 32-lane halves of a wave's 64 dword addresses"""
    worst = 0
    for half in (addrs[:32], addrs[32:]):
        per = {}
        for a in set(half):
            for k in range(width):
                per.setdefault((a + k) % banks, set()).add(a)
        worst = max(worst, max(len(v) for v in per.values()))
    return worst


def test_lds_bank_model_of_the_streamed_layer():
    assert 4 * GS + 36 * XS <= 8 * 4672 and GS % 4 == 0 and GS >= 34 * 34 * 4, "conv0's half and a quarter's V within the activation buffer (37 376 floats)"
    reads, writes, loop = 0, 0, 0
    for wave in range(8):
        for jh in range(2):
            t_in = [((lane >> 1) & 3) * GS + (4 * wave * WP + 4 * (lane >> 3)) * 4 + (lane & 1) + 2 * jh for lane in range(64)]
            for r in range(6):
                for c in range(6):
                    reads = max(reads, _ways([a + (r * WP + c) * 4 for a in t_in], 32))
        t_v = [V + (wave >> 1) * 128 + _slot((lane >> 1) & 3, (wave & 1) * 8 + (lane >> 3)) * 2 + (lane & 1) for lane in range(64)]
        v0 = [V + (wave >> 1) * 128 + _slot(lane >> 4, lane & 15) * 2 for lane in range(64)]
        for xi in range(36):
            writes = max(writes, _ways([a + xi * XS for a in t_v], 32))
            loop = max(loop, _ways([a + xi * XS for a in v0], 64, 2))
    # what a wave's stores cover is what its readers read: every (tile block, kq, m, j) of a position exactly once over the workgroup
    cover = sorted((wave >> 1) * 128 + _slot((lane >> 1) & 3, (wave & 1) * 8 + (lane >> 3)) * 2 + (lane & 1) for wave in range(8) for lane in range(64))
    assert cover == list(range(512))
    print("bank model: transform reads %d-way (a quarter reads half of every 16-byte cell: 16 of 32 banks at best), V stores %d-way, loop reads %d-way" % (reads, writes, loop))
    assert reads == 2 and writes == 1 and loop == 1
    # without the rotation of m by 4 kq the stores would meet 4-way
    plain = [V + (((lane >> 1) & 3) * 16 + (lane >> 3)) * 2 + (lane & 1) for lane in range(64)]
    assert _ways(plain, 32) == 4
