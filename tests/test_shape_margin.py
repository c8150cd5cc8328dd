"""The margin rule of the fused AffNet shape pass (affnet_amd/csrc/shape_filter.h: aff_shape_margin_flag; shape form 1 of affnet_set_shape_form), on the
CPU: the oracle's candidates of the synthetic 320x240 images, seeds 0 .. 5, num_features 300, through the direct fp32 mirror of the AffNet trunk and
through the one with conv1 / conv3 as Winograd F(2x2, 3x3) (tools/winograd_numerics.py).  The library runs the Winograd form on every candidate and the
direct form on the flagged ones, so the rule must flag every candidate whose filter decision differs between the forms - and few others."""
import numpy as np
import pytest

import _shape_margin as sm

SEEDS = (0, 1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def rows(weights):
    """Per seed: frames, pooled head outputs of both forms - computed once, read by every test"""
    out = {}
    for seed in SEEDS:
        patches, lafs = sm.candidates(weights["AffNet"], seed)
        direct, wino = sm.heads(weights["AffNet"], patches)
        out[seed] = {"lafs": lafs.numpy(), "direct": direct, "wino": wino}
    return out


def test_every_decision_that_differs_between_the_forms_is_flagged(rows):
    flips = 0
    for seed in SEEDS:
        r = rows[seed]
        Ad, Aw = sm.a_from_head(r["direct"]), sm.a_from_head(r["wino"])
        differ = sm.filter_decision(Ad, r["lafs"]) != sm.filter_decision(Aw, r["lafs"])
        flag = sm.margin_flag(Aw, r["lafs"])
        iso = (Aw[:, 0] - Aw[:, 3]) ** 2
        print("seed %d: %d candidates, %d decisions differ (largest (o0 - o3)^2 among them %.3g), %d flagged"
              % (seed, len(differ), int(differ.sum()), float(iso[differ].max()) if differ.any() else 0.0, int(flag.sum())))
        assert not (differ & ~flag).any(), "seed %d: rows %s change their decision without a flag" % (seed, np.nonzero(differ & ~flag)[0].tolist())
        flips += int(differ.sum())
    assert flips >= 1, "no decision differs between the forms on these inputs: the test would pass without a rule"


def test_head_outputs_of_the_two_forms_stay_within_delta(rows):
    worst = max(float(np.abs(rows[s]["direct"].astype(np.float64) - rows[s]["wino"]).max()) for s in SEEDS)
    print("largest |Winograd - direct| over the pooled head outputs: %.3g (delta %.3g)" % (worst, sm.DELTA))
    assert worst <= sm.DELTA


def test_flagged_share_per_image_is_small(rows):
    for seed in SEEDS:
        r = rows[seed]
        share = float(sm.margin_flag(sm.a_from_head(r["wino"]), r["lafs"]).mean())
        print("seed %d: flagged share %.2f %%" % (seed, 100 * share))
        assert share <= sm.FLAGGED_SHARE_CAP


def test_non_finite_rows_are_flagged():
    lafs = np.tile(np.array([[0.05, 0.0, 0.5], [0.0, 0.05, 0.5]], dtype=np.float32), (3, 1, 1))
    A = np.array([[np.nan, 0, 0, 1], [1.3, 0, 0.1, 1 / 1.3], [np.inf, 0, 0, 0]], dtype=np.float32)
    lafs[1, 0, 2] = np.nan
    assert sm.margin_flag(A, lafs).all()
    ok = np.array([[1.3, 0, 0.1, 1 / 1.3]], dtype=np.float32)
    assert not sm.margin_flag(ok, lafs[:1]).any()
