"""Helper of tests/test_shape_margin_poly.py: the pooled AffNet head outputs of the direct fp32 trunk and of the trunk that shape form 2 runs on every candidate
(conv1 / conv3 / conv5 as Winograd F(2x2, 3x3), conv2 / conv4 as polyphase F(2x2, 2x2) in the 16-channel kernels' order: tools/winograd_numerics.py). The rule, its
thresholds and the candidates are tests/_shape_margin.py's, unchanged."""
import torch

import _shape_margin as sm
import winograd_numerics as wn

WINO_LAYERS = (1, 3, 5)
POLY_LAYERS = (2, 4)


def heads(sd, patches):
    """Pooled head outputs (n, 3) of the direct fp32 trunk and of shape form 2's first trunk"""
    with torch.no_grad():
        out = []
        for layers, poly in (((), ()), (WINO_LAYERS, POLY_LAYERS)):
            y = wn.trunk16_layers(sd, patches, layers, poly=poly)[5]
            out.append(wn.head16(sd, y, "affnet").numpy().astype(sm.f32))
    return out
