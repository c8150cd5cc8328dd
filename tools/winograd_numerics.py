#!/usr/bin/env python
"""CPU mirror of the Winograd F(2x2, 3x3) layers (affnet_amd/csrc/cnn_mfma.h: conv3x3_wino_mfma for HardNet's conv1 / conv3 / conv5,
conv3x3_wino_mfma_rows for conv1 / conv3 and conv3x3_wino_mfma_half_rows + wino5_combine for conv5 of OriNet; the AffNet mirror prices the same change for AffNet, which stays direct) and the error they add.

The transforms follow the kernel's operation order one add / multiply at a time in the input's dtype:
    U = G g G^T   along x, then y:  s = g0 + g2;  (g0, 0.5 (s + g1), 0.5 (s - g1), g2)
    V = B^T d B   along y, then x:  (d0 - d2, d1 + d2, d2 - d1, d1 - d3)
    Y = A^T M A   along y, then x:  ((m0 + m1) + m2, (m1 - m2) - m3)
The contraction over input channels is one matmul per transform position (the kernel sums it on the fp32 MFMA in its own order; the
summation order changes the last bits, not the size of the error).  BatchNorm is folded into the conv weights and a bias, as the packed
weights of the kernel are.

HardNet's descriptor forms 1 and 2 have their mirrors further down: polyphase F(2x2, 2x2) for conv2 / conv4 (poly_*), F(4x4, 3x3) for conv3 and - form 3 - conv5 (f43_*).

    python tools/winograd_numerics.py [--n 2000]   -> max / mean |descriptor - float64 forward| of direct fp32, Winograd fp32, form 1, form 2 and form 3
    python tools/winograd_numerics.py --net affnet|orinet [--layers 1,3,5]
        -> per trunk layer and at the pooled head output: max |x - float64 forward| of direct fp32 and Winograd fp32 (shipped checkpoints,
           tests/golden/cnn_random_patches.npz and --n smooth seeded patches); OriNet also the error of the angle
"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402

WINO_LAYERS = (1, 3, 5)          # HardNet's stride-1 layers after conv0: conv1, conv3, conv5
WINO_LAYERS_16 = (1, 3, 5)       # OriNet (and the AffNet mirror): conv1, conv3 and conv5.  conv5's two waves per channel block combine their position rows in
                                 # _at_axis's order - (m0 + m1) + m2 in the wave of rows 0, 1, (m1 - m2) - m3 in the wave of rows 2, 3 (cnn_mfma.h: wino5_combine)


def _g_axis(g0, g1, g2):
    s = g0 + g2
    return [g0, 0.5 * (s + g1), 0.5 * (s - g1), g2]


def _bt_axis(d0, d1, d2, d3):
    return [d0 - d2, d1 + d2, d2 - d1, d1 - d3]


def _at_axis(m0, m1, m2, m3):
    return [(m0 + m1) + m2, (m1 - m2) - m3]


def weight_transform(w):
    """w [co][ci][3][3] -> U [4][4][co][ci] (x first, then y)"""
    t = [_g_axis(w[:, :, ky, 0], w[:, :, ky, 1], w[:, :, ky, 2]) for ky in range(3)]       # t[ky][j]
    cols = [_g_axis(t[0][j], t[1][j], t[2][j]) for j in range(4)]                            # cols[j][i]
    return torch.stack([torch.stack([cols[j][i] for j in range(4)]) for i in range(4)])


def input_transform(x):
    """x [n][c][H][H] (H even) -> V [4][4][n][c][H/2][H/2] over the zero-padded 4x4 windows at stride 2 (y first, then x)"""
    xp = F.pad(x, (1, 1, 1, 1))
    H = x.shape[-1]
    d = [[xp[:, :, r:r + H:2, c:c + H:2] for c in range(4)] for r in range(4)]             # d[r][c]: window element (r, c) of every tile
    t = [_bt_axis(d[0][c], d[1][c], d[2][c], d[3][c]) for c in range(4)]                     # t[c][i]
    return torch.stack([torch.stack(_bt_axis(t[0][i], t[1][i], t[2][i], t[3][i])) for i in range(4)])


def wino_conv3x3(x, w):
    """3x3 convolution, padding 1, stride 1 (no bias) as F(2x2, 3x3) in the dtype of x / w: [n][ci][H][H] -> [n][co][H][H]"""
    n, _, H, _ = x.shape
    U = weight_transform(w)                                 # [4][4][co][ci]
    V = input_transform(x)                                  # [4][4][n][ci][HT][HT]
    M = torch.einsum("ijoc,ijncyx->ijnoyx", U, V)           # one contraction over ci per transform position
    t = [_at_axis(M[0, j], M[1, j], M[2, j], M[3, j]) for j in range(4)]                     # t[j][r]
    Y = [[_at_axis(t[0][r], t[1][r], t[2][r], t[3][r])[c] for c in range(2)] for r in range(2)]
    out = torch.empty(n, w.shape[0], H, H, dtype=x.dtype)
    for r in range(2):
        for c in range(2):
            out[:, :, r::2, c::2] = Y[r][c]
    return out


# ---- polyphase Winograd F(2x2, 2x2) of the stride-2 layers (HardNet form 1: conv2 / conv4; cnn_mfma.h: conv3x3_poly_mfma_rows) ----------------
# Along an axis output o of a 3x3 stride-2 padding-1 convolution reads inputs 2 o - 1, 2 o, 2 o + 1: taps 0 and 2 fall on odd samples, tap 1 on an even
# one.  Over the 5 samples d0 .. d4 of two outputs the odd phase is a 2-tap stride-1 filter (g0, g2) on (d0, d2, d4), run as F(2, 2):
#     m0 = (d0 - d2) g0,  m1 = d2 (g0 + g2),  m2 = (d2 - d4) g2;   y0 = m0 + m1,  y1 = m1 - m2
# and the even phase adds n0 = d1 g1 to y0 and n1 = d3 g1 to y1.  An axis index 0 .. 2 is an odd-phase product, 3 .. 4 an even-phase one; the 25 products
# of a 2x2 output tile are numbered xi = 3 i + j (odd rows, odd columns), 9 + 2 i + j (odd rows, even columns), 15 + 3 i + j (even rows, odd columns),
# 21 + 2 i + j (even rows, even columns), i / j counting inside the phase.
def _pg_axis(g0, g1, g2):
    return [g0, g0 + g2, g2, g1, g1]


def _pb_axis(d0, d1, d2, d3, d4):
    return [d0 - d2, d2, d2 - d4, d1, d3]


def _po_axis(m0, m1, m2, n0, n1):
    return [(m0 + m1) + n0, (m1 - m2) + n1]


def poly_xi(iy, ix):
    """position number of the axis indices (iy, ix), each 0 .. 2 odd phase, 3 .. 4 even phase"""
    if iy < 3:
        return 3 * iy + ix if ix < 3 else 9 + 2 * iy + (ix - 3)
    return 15 + 3 * (iy - 3) + ix if ix < 3 else 21 + 2 * (iy - 3) + (ix - 3)


def poly_weight_transform(w):
    """w [co][ci][3][3] -> U [25][co][ci] (x first, then y): every entry is a tap or a sum of two along each axis"""
    t = [_pg_axis(w[:, :, ky, 0], w[:, :, ky, 1], w[:, :, ky, 2]) for ky in range(3)]      # t[ky][ix]
    cols = [_pg_axis(t[0][ix], t[1][ix], t[2][ix]) for ix in range(5)]                       # cols[ix][iy]
    U = [None] * 25
    for iy in range(5):
        for ix in range(5):
            U[poly_xi(iy, ix)] = cols[ix][iy]
    return torch.stack(U)


def poly_input_transform(x):
    """x [n][c][H][H] (H a multiple of 4) -> V [25][n][c][H/4][H/4] over the zero-padded 5x5 windows at stride 4 (y first, then x)"""
    xp = F.pad(x, (1, 1, 1, 1))
    H = x.shape[-1]
    d = [[xp[:, :, r:r + H:4, c:c + H:4] for c in range(5)] for r in range(5)]             # d[r][c]: window element (r, c) of every tile
    t = [_pb_axis(*[d[r][c] for r in range(5)]) for c in range(5)]                           # t[c][iy]
    V = [None] * 25
    for iy in range(5):
        row = _pb_axis(*[t[c][iy] for c in range(5)])
        for ix in range(5):
            V[poly_xi(iy, ix)] = row[ix]
    return torch.stack(V)


def poly_conv3x3_s2(x, w):
    """3x3 convolution, padding 1, stride 2 (no bias) as polyphase F(2x2, 2x2) in the dtype of x / w: [n][ci][H][H] -> [n][co][H/2][H/2]"""
    n, _, H, _ = x.shape
    U = poly_weight_transform(w)                            # [25][co][ci]
    V = poly_input_transform(x)                             # [25][n][ci][H/4][H/4]
    M = torch.einsum("poc,pncyx->pnoyx", U, V)              # one contraction over ci per position
    t = [_po_axis(*[M[poly_xi(iy, ix)] for iy in range(5)]) for ix in range(5)]              # t[ix][dy]: rows first ...
    out = torch.empty(n, w.shape[0], H // 2, H // 2, dtype=x.dtype)
    for dy in range(2):
        Y = _po_axis(*[t[ix][dy] for ix in range(5)])                                        # ... then columns
        for dx in range(2):
            out[:, :, dy::2, dx::2] = Y[dx]
    return out


def poly_packed_weight_transform(sd, layers=(2, 4)):
    """{layer: U} of HardNet's stride-2 layers as derive_u_kernel leaves them (affnet_amd/csrc/weights_layout.h: derived_hardnet_poly, poly_weight_transform, w_tap_index over 25
    positions): flat float32 [xi (25)][ci / 16][(c / 4) % 4][co][c % 4] of the BN-folded fp32 taps"""
    out = {}
    for i in layers:
        U = poly_weight_transform(packed_taps(sd, i))        # [25][co][ci]
        co, ci = U.shape[1:]
        out[i] = U.reshape(25, co, ci // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)
    return out


POLY_LAYERS = (2, 4)             # HardNet's stride-2 layers


# ---- the same form in the 16-channel trunks (AffNet shape form 2, exact OriNet; cnn_mfma.h: conv3x3_poly16_mfma_rows, poly16_combine) -------------------------
# conv2 (16 -> 32 @32x32 -> 16x16) has ONE K group of 16 input channels: a wave runs the ten position rows of its (tile block, channel block) unit and folds them as
# poly_conv3x3_s2 does.  conv4 (32 -> 64 @16x16 -> 8x8) has two K groups and a wave pair per channel block: each wave runs the ten position rows over ITS 16 input
# channels and folds them into a partial y, and the pair adds the partial y in the order K group 0 + K group 1.
def poly16_conv2(x, w):
    assert x.shape[1] == 16
    return poly_conv3x3_s2(x, w)


def poly16_conv4(x, w):
    assert x.shape[1] == 32
    return poly_conv3x3_s2(x[:, :16], w[:, :16]) + poly_conv3x3_s2(x[:, 16:], w[:, 16:])


def poly16_conv(li, x, w):
    return poly16_conv2(x, w) if li == 2 else poly16_conv4(x, w)


def poly16_packed_weight_transform(sd, layers=(2, 4)):
    """{layer: U} of the stride-2 layers of an AffNet / OriNet state dict as derive_u_kernel leaves them behind the Winograd sections (Wino16::offset(2 / 4)):
    the layout of poly_packed_weight_transform, 25 x 16 x 32 and 25 x 32 x 64 floats"""
    return poly_packed_weight_transform(sd, layers)


# ---- Winograd F(4x4, 3x3), points 0, +-1, +-2 (HardNet form 2: conv3; cnn_mfma.h: conv3x3_f43_mfma_shared_v + f43_combine) ---------------------------
# Per axis, one rounding per operation, in the kernel's order (cnn_mfma.h: f43_bt_lo / f43_bt_hi / f43_at_axis, weights_layout.h: f43_g_axis):
#     U = G g:    s = g0 + g2;  p = (1/24) g0 + (1/6) g2;  q = (1/12) g1:   (0.25 g0, (-1/6)(s + g1), (-1/6)(s - g1), p + q, p - q, g2)
#     V = B^T d:  (4 d0 - 5 d2) + d4;  a = d4 - 4 d2, b = d3 - 4 d1: a + b, a - b;  c = d4 - d2, e = 2 (d3 - d1): c + e, c - e;  (4 d1 - 5 d3) + d5
#     Y = A^T m:  p = m1 + m2, q = m1 - m2, r = m3 + m4, s = m3 - m4:  (m0 + p) + r,  q + 2 s,  p + 4 r,  q + (8 s + m5)
# The weights along x, then y; the input along y, then x; the output along x, then y (in the kernel the y stage is split over a wave pair: f43_combine forms these sums).
def _f43_const(v, like):
    return torch.tensor(v, dtype=like.dtype)


def _f43_g_axis(g0, g1, g2):
    # the kernel's constants are the floats nearest to 1/6, 1/12, 1/24 (1.0f / 6.0f ...); in float64 the doubles nearest to them
    c6, c12, c24 = (_f43_const(1.0 / k, g0) for k in (6.0, 12.0, 24.0))
    s = g0 + g2
    p = c24 * g0 + c6 * g2
    q = c12 * g1
    return [0.25 * g0, (-c6) * (s + g1), (-c6) * (s - g1), p + q, p - q, g2]


def _f43_bt_axis(d0, d1, d2, d3, d4, d5):
    a, b = d4 - 4.0 * d2, d3 - 4.0 * d1
    c, e = d4 - d2, 2.0 * (d3 - d1)
    return [(4.0 * d0 - 5.0 * d2) + d4, a + b, a - b, c + e, c - e, (4.0 * d1 - 5.0 * d3) + d5]


def _f43_at_axis(m0, m1, m2, m3, m4, m5):
    p, q, r, s = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    return [(m0 + p) + r, q + 2.0 * s, p + 4.0 * r, q + (8.0 * s + m5)]


def f43_weight_transform(w):
    """w [co][ci][3][3] -> U [36][co][ci], xi = 6 i + j (x first, then y)"""
    t = [_f43_g_axis(w[:, :, ky, 0], w[:, :, ky, 1], w[:, :, ky, 2]) for ky in range(3)]   # t[ky][j]
    cols = [_f43_g_axis(t[0][j], t[1][j], t[2][j]) for j in range(6)]                        # cols[j][i]
    return torch.stack([cols[j][i] for i in range(6) for j in range(6)])


def f43_input_transform(x):
    """x [n][c][H][H] (H a multiple of 4) -> V [36][n][c][H/4][H/4] over the zero-padded 6x6 windows at stride 4 (y first, then x)"""
    xp = F.pad(x, (1, 1, 1, 1))
    H = x.shape[-1]
    d = [[xp[:, :, r:r + H:4, c:c + H:4] for c in range(6)] for r in range(6)]             # d[r][c]: window element (r, c) of every tile
    t = [_f43_bt_axis(*[d[r][c] for r in range(6)]) for c in range(6)]                       # t[c][i]
    return torch.stack([v for i in range(6) for v in _f43_bt_axis(*[t[c][i] for c in range(6)])])


def f43_conv3x3(x, w):
    """3x3 convolution, padding 1, stride 1 (no bias) as F(4x4, 3x3) in the dtype of x / w: [n][ci][H][H] -> [n][co][H][H]"""
    n, _, H, _ = x.shape
    U = f43_weight_transform(w)                             # [36][co][ci]
    V = f43_input_transform(x)                              # [36][n][ci][H/4][H/4]
    M = torch.einsum("poc,pncyx->pnoyx", U, V)              # one contraction over ci per position
    t = [_f43_at_axis(*[M[6 * i + j] for j in range(6)]) for i in range(6)]                  # t[i][c]: columns first ...
    out = torch.empty(n, w.shape[0], H, H, dtype=x.dtype)
    for c in range(4):
        Y = _f43_at_axis(*[t[i][c] for i in range(6)])                                       # ... then rows
        for r in range(4):
            out[:, :, r::4, c::4] = Y[r]
    return out


def f43_packed_weight_transform(sd, layers=(1, 3)):
    """{layer: U} of HardNet's conv1 / conv3 as derive_u_kernel leaves them (affnet_amd/csrc/weights_layout.h: derived_hardnet_f43, f43_weight_transform, w_tap_index over 36
    positions): flat float32 [xi (36)][ci / 16][(c / 4) % 4][co][c % 4] of the BN-folded fp32 taps"""
    out = {}
    for i in layers:
        U = f43_weight_transform(packed_taps(sd, i))         # [36][co][ci]
        co, ci = U.shape[1:]
        out[i] = U.reshape(36, co, ci // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)
    return out


F43_LAYERS = (3,)                # the layers HardNet's descriptor form 2 runs as F(4x4, 3x3)
F43_LAYERS_FORM3 = (3, 5)        # ... and descriptor form 3: conv5 as well, in a kernel of its own (affnet_amd/csrc/hardnet_conv5_f43.hip)
F43_LAYERS_FORM4 = (1, 3, 5)     # ... and descriptor form 4: conv1 as well, streamed with conv0 over its K (affnet_amd/csrc/cnn_trunk.h: STREAM1) - every accumulator sums
                                 # its K in the order f43_conv3x3's contraction stands for (K group ascending, k-step ascending), lane-local transforms on both sides


def f43_conv5_grouped(x, w):
    """conv5 of descriptor form 3 (hardnet_conv5_f43_kernel): 128 -> 128 at 8 x 8, the four 4x4 tiles of a patch, four patches per workgroup.  A patch's result does not
    depend on its group: every accumulator (tile, cout, position) sums its own 128 products, lane-local transforms on both sides (cnn_mfma.h: f43c5_transform = f43_bt_lo /
    f43_bt_hi along y, then x; f43c5_output = f43_at_axis along x, then y), so the mirror is f43_conv3x3 at this shape - with its one contraction per position, as everywhere here"""
    assert tuple(x.shape[1:]) == (128, 8, 8) and tuple(w.shape) == (128, 128, 3, 3)
    return f43_conv3x3(x, w)


def f43_conv5_packed_weight_transform(sd):
    """U of conv5 as derive_u_kernel leaves it for descriptor form 3 (weights_layout.h: derived_hardnet_form3, F43C5): flat float32 [xi (36)][8][(c / 4) % 4][128][c % 4]"""
    return f43_packed_weight_transform(sd, layers=(5,))[5]


def folded(sd, dtype):
    """BatchNorm (eval, affine=False, eps 1e-5) folded into the six conv layers: [(weight, bias, stride)]"""
    layers = []
    for ci, bi, st in orc._TRUNK:
        w = sd["features.%d.weight" % ci].to(dtype)
        inv = 1.0 / torch.sqrt(sd["features.%d.running_var" % bi].to(dtype) + 1e-5)
        layers.append((w * inv.view(-1, 1, 1, 1), -sd["features.%d.running_mean" % bi].to(dtype) * inv, st))
    return layers


def packed_taps(sd, i):
    """BN-folded fp32 taps [co][ci][3][3] of trunk layer i with the packer's own roundings (affnet_amd/csrc/weights_pack.hip: fold_bn,
    w * (1.0f / sqrtf(var + 1e-5f)), every operation correctly rounded - numpy's float32 sqrt and divide are; torch's vectorised CPU sqrt is
    an ulp off on a few inputs, which is why `folded` above is not used where bits are compared)"""
    import numpy as np
    ci, bi, _ = orc._TRUNK[i]
    var = sd["features.%d.running_var" % bi].detach().to(torch.float32).numpy()
    inv = np.float32(1.0) / np.sqrt(var + np.float32(1e-5))
    w = sd["features.%d.weight" % ci].detach().to(torch.float32).numpy() * inv.reshape(-1, 1, 1, 1)
    assert w.dtype == np.float32
    return torch.from_numpy(w)


def packed_weight_transform(sd):
    """{layer: U} of HardNet's Winograd layers as the packed blob stores them (affnet_amd/csrc/weights_layout.h: NetLayout::w_wino,
    w_tap_index; affnet_cnn32_winograd_offset): the fp32 weight_transform of the BN-folded fp32 taps (the mirror of that header's
    wino_weight_transform), flat float32 [xi = 4 i + j (16)][ci / 16][(c / 4) % 4][co][c % 4]"""
    out = {}
    for i in WINO_LAYERS:
        U = weight_transform(packed_taps(sd, i))             # [4][4][co][ci]
        co, ci = U.shape[2:]
        out[i] = U.reshape(16, co, ci // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)
    return out


def hardnet_forward(sd, patches, wino=True, dtype=torch.float32, poly=False, f43=()):
    """HardNet descriptors in `dtype`; conv1 / conv3 / conv5 as Winograd when `wino`, conv2 / conv4 as polyphase F(2x2, 2x2) when `poly`, the layers in `f43`
    (of 1, 3, 5; descriptor form 2: F43_LAYERS, form 3: F43_LAYERS_FORM3) as F(4x4, 3x3) instead of F(2x2, 3x3)"""
    x = orc.input_norm(patches.to(dtype))
    for li, (w, b, st) in enumerate(folded(sd, dtype)):
        if poly and li in POLY_LAYERS:
            y = poly_conv3x3_s2(x, w)
        elif li in f43:
            y = f43_conv5_grouped(x, w) if li == 5 else f43_conv3x3(x, w)
        else:
            y = wino_conv3x3(x, w) if (wino and li in WINO_LAYERS) else F.conv2d(x, w, None, stride=st, padding=1)
        x = F.relu(y + b.view(1, -1, 1, 1))
    y = F.conv2d(x, sd["features.19.weight"].to(dtype), None)
    y = F.batch_norm(y, sd["features.20.running_mean"].to(dtype), sd["features.20.running_var"].to(dtype), None, None, False, 0.1, 1e-5)
    y = y.view(y.size(0), -1)
    return y / torch.sqrt(torch.sum(y * y, dim=1) + 1e-8).unsqueeze(-1)


def trunk16_layers(sd, patches, layers=WINO_LAYERS_16, dtype=torch.float32, poly=()):
    """The six post-ReLU trunk tensors of AffNet / OriNet in `dtype`, the layers in `layers` as Winograd (() = all direct), those in `poly` (of 2, 4) as polyphase
    F(2x2, 2x2) in the 16-channel kernels' order (AffNet shape form 2 and the exact OriNet trunk: POLY_LAYERS)"""
    x = orc.input_norm(patches.to(dtype))
    outs = []
    for li, (w, b, st) in enumerate(folded(sd, dtype)):
        if li in poly:
            y = poly16_conv(li, x, w)
        else:
            y = wino_conv3x3(x, w) if li in layers else F.conv2d(x, w, None, stride=st, padding=1)
        x = F.relu(y + b.view(1, -1, 1, 1))
        outs.append(x)
    return outs


def head16(sd, y, net, dtype=torch.float32):
    """Pooled head output: AffNet (n, 3) - the numbers A is built from; OriNet (n, 2) - the vector whose atan2 is the angle"""
    y = torch.tanh(F.conv2d(y, sd["features.19.weight"].to(dtype), sd["features.19.bias"].to(dtype), padding=1 if net == "orinet" else 0))
    return F.adaptive_avg_pool2d(y, 1).flatten(1)


def errors16(sd, patches, net, layers=WINO_LAYERS_16):
    """{"direct" | "winograd" | "polyphase" (Winograd + conv2 / conv4 polyphase): {"layers": [6 x max |x - fp64| / max(1, |fp64|max)], "head": max |head - fp64|, "angle": rad (OriNet)}}"""
    with torch.no_grad():
        ref = trunk16_layers(sd, patches, (), torch.float64)
        href = head16(sd, ref[5], net, torch.float64)
        out = {}
        for name, ls, pl in (("direct", (), ()), ("winograd", tuple(layers), ()), ("polyphase", tuple(layers), POLY_LAYERS)):
            got = trunk16_layers(sd, patches, ls, poly=pl)
            h = head16(sd, got[5], net)
            rec = {"layers": [float((g.double() - r).abs().max()) / max(1.0, float(r.abs().max())) for g, r in zip(got, ref)],
                   "head": float((h.double() - href).abs().max())}
            if net == "orinet":
                ang = lambda v: torch.atan2(v[:, 0] + 1e-8, v[:, 1] + 1e-8)
                d = ang(h).double() - ang(href)
                rec["angle"] = float(((d + math.pi) % (2 * math.pi) - math.pi).abs().max())
            out[name] = rec
    return out


def smooth_patches(n, seed=1):
    """n seeded smooth patches (8 x 8 noise, bilinear to 32 x 32) - closer to image content than white noise"""
    return F.interpolate(torch.rand(n, 1, 8, 8, generator=torch.Generator().manual_seed(seed)) * 255, size=32, mode="bilinear")


def load_net16(net):
    name = {"affnet": "AffNet", "orinet": "OriNet"}[net]
    return torch.load(os.path.join(ROOT, "pretrained", name + ".pth"), map_location="cpu", weights_only=False)["state_dict"]


def errors(sd, patches):
    """(max, mean) |descriptor - float64 forward| of direct fp32, of Winograd fp32, of Winograd + polyphase fp32 (form 1), of form 2 (conv3 as F(4x4, 3x3)) and of form 3 (conv5 as well)"""
    with torch.no_grad():
        ref = orc.hardnet_forward({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, patches.double())
        out = {}
        for name, wino, poly, f43 in (("direct", False, False, ()), ("winograd", True, False, ()), ("polyphase", True, True, ()), ("f43", True, True, F43_LAYERS), ("f43_conv5", True, True, F43_LAYERS_FORM3), ("f43_conv1", True, True, F43_LAYERS_FORM4)):
            d = (hardnet_forward(sd, patches, wino=wino, poly=poly, f43=f43).double() - ref).abs()
            out[name] = (float(d.max()), float(d.mean()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--net", choices=("hardnet", "affnet", "orinet"), default="hardnet")
    ap.add_argument("--layers", default="1,3,5", help="Winograd layers of the AffNet / OriNet mirror")
    args = ap.parse_args()
    if args.net != "hardnet":
        import numpy as np
        sd = load_net16(args.net)
        layers = tuple(int(v) for v in args.layers.split(","))
        golden = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "cnn_random_patches.npz"))["patches"]).reshape(-1, 1, 32, 32)
        print("%s, Winograd in layers %s; max abs error vs float64 (layers: relative to max(1, |ref|max))" % (args.net, layers))
        for tag, p in (("golden random", golden), ("%d smooth" % args.n, smooth_patches(args.n, args.seed + 1))):
            e = errors16(sd, p, args.net, layers)
            for k in ("direct", "winograd", "polyphase"):
                print("%-14s %-9s layers %s  head %.3g%s" % (tag, k, " ".join("%.2g" % v for v in e[k]["layers"]), e[k]["head"],
                                                           "  angle %.3g rad" % e[k]["angle"] if "angle" in e[k] else ""))
        return
    sd = orc.synthetic_hardnet_state(0)
    p = torch.rand(args.n, 1, 32, 32, generator=torch.Generator().manual_seed(args.seed)) * 255
    for name, (mx, mean) in errors(sd, p).items():
        print("%-9s max %.3g  mean %.3g" % (name, mx, mean))


if __name__ == "__main__":
    main()
