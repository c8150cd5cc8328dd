"""CPU side of tests/test_gpu_handcrafted.py: the conditions the patch families of tests/_handcrafted_fp64.py must meet for the GPU test
to be fair, and the reference's own fp32 error that sets the GPU test's Baumberg bar.  A narrower fixture fails here, loudly."""
import numpy as np
import pytest
import torch

import _handcrafted_fp64 as hc
import affnet_oracle as orc
from conftest import record_parity


@pytest.fixture(scope="module")
def fam():
    patches, names, family = hc.families()
    return patches, names, family, hc.orientation_f64(patches)


def test_families_are_what_they_claim(fam):
    patches, names, family, _ = fam
    assert patches.shape == (286, 1, 19, 19) and patches.dtype == np.float32 and len(names) == len(set(names)) == 286
    assert [int((family == f).sum()) for f in "abcde"] == [36, 100, 100, 2, 48]
    again = hc.families()[0]
    assert np.array_equal(again, patches)                                       # deterministic
    assert patches[family != "e"].min() >= 0.0 and patches[family != "e"].max() <= 255.0
    assert np.all(patches[family == "d"][0] == 77.0) and not patches[family == "d"][1].any()


def test_orientation_fixture_conditions(fam):
    """Decided patches cover all 36 bins; undecided ones are at most 5 % of families a - d; the fp32 oracle agrees with the float64
    restatement on every decided patch and stays inside the restatement's two largest bins on every other."""
    patches, names, family, r = fam
    synth = family != "e"
    dec = r["decided"]
    covered = sorted(set(r["bin"][dec].tolist()))
    undecided = [names[i] for i in np.nonzero(synth & ~dec)[0]]
    share = len(undecided) / float(synth.sum())
    bins32 = hc.oracle_orientation_bins(patches)
    wrong = [names[i] for i in np.nonzero(dec & (bins32 != r["bin"]))[0]]
    stray = [names[i] for i in np.nonzero(~dec & (bins32 != r["top2"][:, 0]) & (bins32 != r["top2"][:, 1]))[0]]
    print("orientation fixture: %d undecided of %d synthetic patches (%.1f %%): %s; %d undecided golden; bins covered %d; fp32/fp64 "
          "disagreements on decided patches %d" % (len(undecided), synth.sum(), 100 * share, undecided, int((~dec & ~synth).sum()), len(covered), len(wrong)))
    record_parity("hand-crafted orientation fixture (host)", patches=int(len(names)), undecided_synthetic=len(undecided), undecided_share=share,
                  undecided_golden=int((~dec & ~synth).sum()), bins_covered=len(covered), fp32_fp64_disagreements_on_decided=len(wrong))
    assert covered == list(range(36)), "bins reached by decided patches: %s" % covered
    assert share <= 0.05, undecided
    assert not wrong, wrong
    assert not stray, stray
    # the ramps' interior gradient sits mid-bin k (the replicate border halves one component there, so the smoothed maximum may move
    # to a neighbour): bins 0 and 35 - the zero-padded ends of the smoothing - are reached by decided ramps
    ramp = np.nonzero((family == "a") & dec)[0]
    assert {0, 35} <= set(r["bin"][ramp].tolist()), r["bin"][ramp].tolist()
    # the constant patches: every pixel has atan2(0, 0) = 0, o_big = 18 exactly - on an integer, hence undecided by construction
    flat = np.nonzero(family == "d")[0]
    assert not dec[flat].any() and np.all(r["n_near"][flat] == 361) and np.all(r["bin"][flat] == 18)
    # the kernel's angle formula restated: the bin is recoverable from the angle
    assert np.array_equal(hc.bin_of_angle(r["angle"]), r["bin"])
    a32 = orc.orientation_detector(torch.from_numpy(patches)).numpy()
    assert np.abs(a32[dec] - r["angle"][dec]).max() < 1e-6


def test_tolerance_leaves_a_factor_of_ten(fam, monkeypatch):
    """With TOL = 1e-5 no more patches are undecided than the two constant ones plus those of TOL = 1e-4: the flagged set shrinks, so 1e-4
    is not at the edge of the host's own rounding."""
    patches, names, family, r = fam
    synth = family != "e"
    monkeypatch.setattr(hc, "TOL", 1e-5)
    tight = hc.orientation_f64(patches)
    assert not (tight["decided"] < r["decided"]).any()                        # decided at 1e-4 => decided at 1e-5
    print("undecided synthetic patches at TOL 1e-5: %d" % int((synth & ~tight["decided"]).sum()))
    assert np.array_equal(tight["bin"], r["bin"])


def test_baumberg_reference_error_and_fixture_conditions(fam):
    """e_ref per family = the fp32 oracle against the float64 restatement on well-conditioned patches (recorded: the GPU bar is 8 x);
    b and c are well-conditioned throughout; the ramps are rank 1; the constant patches are non-finite in the oracle's fp32 result."""
    patches, names, family, _ = fam
    e_ref, got, want, eig = hc.baumberg_reference_error(patches, family)
    ok = hc.well_conditioned(eig)
    assert ok[family == "b"].all() and ok[family == "c"].all()
    assert int(ok[family == "e"].sum()) >= 40, int(ok[family == "e"].sum())
    assert not ok[family == "a"].any()                                          # rank-1 moment matrices: only the output's shape is asserted
    aniso = np.sqrt(eig[:, 1] / np.maximum(eig[:, 0], 1e-300))
    print("Baumberg e_ref: %s; anisotropy up to %.1f (b), %.1f (c)" % ({k: "%.3g over %d" % v for k, v in e_ref.items()},
                                                                       aniso[family == "b"].max(), aniso[family == "c"].max()))
    record_parity("hand-crafted Baumberg: the reference's own fp32 error (host)", **{"e_ref_" + k: v[0] for k, v in e_ref.items()},
                  **{"patches_" + k: v[1] for k, v in e_ref.items()}, anisotropy_max_c=float(aniso[family == "c"].max()))
    for k, (e, cnt) in e_ref.items():
        assert 0.0 < e < 1e-5, (k, e)                                           # fp32 rounding of values of order 1, nothing more
    flat = family == "d"
    assert (~np.isfinite(got[flat]).all(axis=(1, 2))).all() and (~np.isfinite(want[flat]).all(axis=(1, 2))).all()
    ramp = family == "a"
    fin = np.isfinite(got[ramp]).all(axis=(1, 2))
    assert np.all(got[ramp][fin][:, 0, 1] == 0.0)
    # up is up on every finite row
    finite = np.isfinite(want).all(axis=(1, 2))
    assert np.all(want[finite][:, 0, 1] == 0.0) and np.allclose(want[finite & ok][:, 0, 0] * want[finite & ok][:, 1, 1], 1.0, rtol=1e-6)
