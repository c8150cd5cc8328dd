"""The margin rule of the fused AffNet shape pass (affnet_amd/csrc/shape_filter.h: aff_shape_margin_flag) with conv5 of the Winograd trunk as F(2x2, 3x3) too:
tests/test_shape_margin.py's three data tests with the Winograd fp32 mirror taken at layers (1, 3, 5) (tools/winograd_numerics.py), which is what the first
trunk of shape form 1 runs.  Same candidates (the oracle's, synthetic 320x240 images, seeds 0 .. 5, num_features 300), same rule, same thresholds: every
decision that differs between this form and the direct one must be flagged, the pooled head outputs must stay within the delta the rule assumes, and the
flagged share must stay small."""
import numpy as np
import pytest
import torch

import _shape_margin as sm
import winograd_numerics as wn

SEEDS = (0, 1, 2, 3, 4, 5)
WINO_LAYERS = (1, 3, 5)


def heads(sd, patches):
    """Pooled head outputs (n, 3) of the direct fp32 trunk and of the one with conv1 / conv3 / conv5 as Winograd"""
    with torch.no_grad():
        out = []
        for layers in ((), WINO_LAYERS):
            y = wn.trunk16_layers(sd, patches, layers)[5]
            out.append(wn.head16(sd, y, "affnet").numpy().astype(sm.f32))
    return out


@pytest.fixture(scope="module")
def rows(weights):
    """Per seed: frames, pooled head outputs of both forms - computed once, read by every test"""
    out = {}
    for seed in SEEDS:
        patches, lafs = sm.candidates(weights["AffNet"], seed)
        direct, wino = heads(weights["AffNet"], patches)
        out[seed] = {"lafs": lafs.numpy(), "direct": direct, "wino": wino}
    return out


def test_every_decision_that_differs_between_the_forms_is_flagged(rows):
    flips = 0
    for seed in SEEDS:
        r = rows[seed]
        Ad, Aw = sm.a_from_head(r["direct"]), sm.a_from_head(r["wino"])
        differ = sm.filter_decision(Ad, r["lafs"]) != sm.filter_decision(Aw, r["lafs"])
        flag = sm.margin_flag(Aw, r["lafs"])
        print("seed %d: %d candidates, %d decisions differ, %d flagged" % (seed, len(differ), int(differ.sum()), int(flag.sum())))
        assert not (differ & ~flag).any(), "seed %d: rows %s change their decision without a flag" % (seed, np.nonzero(differ & ~flag)[0].tolist())
        flips += int(differ.sum())
    assert flips >= 1, "no decision differs between the forms on these inputs: the test would pass without a rule"


def test_head_outputs_of_the_two_forms_stay_within_delta(rows):
    worst = max(float(np.abs(rows[s]["direct"].astype(np.float64) - rows[s]["wino"]).max()) for s in SEEDS)
    print("largest |Winograd(1, 3, 5) - direct| over the pooled head outputs: %.3g (delta %.3g)" % (worst, sm.DELTA))
    assert worst <= sm.DELTA


def test_flagged_share_per_image_is_small(rows):
    for seed in SEEDS:
        r = rows[seed]
        share = float(sm.margin_flag(sm.a_from_head(r["wino"]), r["lafs"]).mean())
        print("seed %d: flagged share %.2f %%" % (seed, 100 * share))
        assert share <= sm.FLAGGED_SHARE_CAP
