"""The margin rule of the fused AffNet shape pass (affnet_amd/csrc/shape_filter.h: aff_shape_margin_flag) under shape form 2, whose first trunk runs layers 1 .. 5 in
reduced-product forms: conv1 / conv3 / conv5 as Winograd F(2x2, 3x3) and conv2 / conv4 as polyphase F(2x2, 2x2) (tests/_shape_margin_poly.py, the fp32 mirrors of
tools/winograd_numerics.py).  tests/test_shape_margin_conv5.py's three data tests on the same candidates (the oracle's, synthetic 320x240 images, seeds 0 .. 5,
num_features 300 -> 450 candidates each), the same rule and thresholds: every decision that differs between this form and the direct one must be flagged, the pooled
head outputs must stay within the delta the rule assumes (4e-6; form 1 measured 3.6e-7), and the flagged share is reported (form 1: 1.3 to 2.9 %)."""
import numpy as np
import pytest

import _shape_margin as sm
import _shape_margin_poly as smp

SEEDS = (0, 1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def rows(weights):
    """Per seed: frames, pooled head outputs of both forms - computed once, read by every test"""
    out = {}
    for seed in SEEDS:
        patches, lafs = sm.candidates(weights["AffNet"], seed)
        assert patches.shape[0] == 450
        direct, form2 = smp.heads(weights["AffNet"], patches)
        out[seed] = {"lafs": lafs.numpy(), "direct": direct, "form2": form2}
    return out


def test_every_decision_that_differs_between_the_forms_is_flagged(rows):
    for seed in SEEDS:
        r = rows[seed]
        Ad, A2 = sm.a_from_head(r["direct"]), sm.a_from_head(r["form2"])
        differ = sm.filter_decision(Ad, r["lafs"]) != sm.filter_decision(A2, r["lafs"])
        flag = sm.margin_flag(A2, r["lafs"])
        print("seed %d: %d candidates, %d decisions differ, %d flagged" % (seed, len(differ), int(differ.sum()), int(flag.sum())))
        assert not (differ & ~flag).any(), "seed %d: rows %s change their decision without a flag" % (seed, np.nonzero(differ & ~flag)[0].tolist())


def test_head_outputs_of_the_two_forms_stay_within_delta(rows):
    worst = max(float(np.abs(rows[s]["direct"].astype(np.float64) - rows[s]["form2"]).max()) for s in SEEDS)
    print("largest |form 2 - direct| over the pooled head outputs: %.3g (delta %.3g)" % (worst, sm.DELTA))
    assert worst < sm.DELTA


def test_flagged_share_per_image_is_reported_and_small(rows):
    for seed in SEEDS:
        r = rows[seed]
        share = float(sm.margin_flag(sm.a_from_head(r["form2"]), r["lafs"]).mean())
        print("seed %d: flagged share %.2f %%" % (seed, 100 * share))
        assert share <= sm.FLAGGED_SHARE_CAP
