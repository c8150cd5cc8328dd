"""CPU side of the caller-supplied-frames feature: the host ellipse reader, the fixture it is checked against, and the margins of the
oracle decisions that tests/test_gpu_frames.py relies on (checked wherever the CPU suite runs)."""
import numpy as np

import _frames as fr


def test_float64_restatement_pins_the_fixture():
    """tests/golden/ells2lafs.npz is the unmodified reference's fp32 ells2LAFsT output.  Its distance from the same formulas in float64
    is a few fp32 roundings of a chain of ~25 operations, each <= 2^-24 relative (measured 4.85e-7 of the frame scale on the authoring
    host): anything above 25 * 2^-24 = 1.5e-6 means the fixture or the restatement is not what it claims to be."""
    ells, lafs, bar, _, m = fr.golden_ells()
    assert ells.shape == (603, 5) and lafs.shape == (603, 2, 3) and ells.dtype == np.float32 and lafs.dtype == np.float32
    assert int((ells[:, 3] == 0).sum()) == 3                                   # the three hand-made rows of the b == 0 branch
    assert 0 < m["reference_own_error"] < 25 * 2.0 ** -24, m
    want = fr.ells2lafs_f64(ells)
    assert np.array_equal(want[:, :, 2].astype(np.float32), lafs[:, :, 2])        # centres pass through
    assert np.all(lafs[:, 0, 1] == 0)                                          # up is up
    # the hand-made rows are known in closed form: radius 10; axes (5, 20); axes (40, 4)
    assert np.allclose(want[-3:, [0, 1], [0, 1]], [[10, 10], [5, 20], [40, 4]], rtol=1e-6) and np.all(want[-3:, 1, 0] == 0)


def test_host_ells2lafs_against_the_golden():
    """affnet_amd.LAF.ells2LAFs (numpy, float64 arithmetic) within 8 x the reference's own fp32 error of the reference's output."""
    from affnet_amd import LAF
    ells, lafs, bar, _, m = fr.golden_ells()
    got = LAF.ells2LAFs(ells.astype(np.float64))
    err = fr.shape_err(got, lafs)
    print("host ells2LAFs vs golden: worst %.3g of the frame scale, bar %.3g" % (err.max(), bar))
    assert err.max() <= bar, (err.max(), bar)
    assert np.array_equal(got[:, :, 2].astype(np.float32), lafs[:, :, 2])
    one = LAF.Ell2LAF(ells[0].astype(np.float64))
    assert np.array_equal(one, got[0])
    a, b, c = LAF.invSqrt(np.float64(0.04), np.float64(0.0), np.float64(0.0025))   # diag(25, 400)^-1 -> diag(5, 20) / 10
    assert abs(a - 0.5) < 1e-12 and b == 0 and abs(c - 2.0) < 1e-12


def test_oracle_decisions_on_the_foreign_frames_have_margin(weights):
    """The frames of test_gpu_frames.py::test_foreign_frames_against_the_oracle: no shape-filter decision of the oracle is close enough to
    its threshold for an fp32 reordering of the CNN sums (~1e-5 relative at AffNet's output) to flip it - so the GPU test may demand the
    SAME set of rows."""
    for n_out in (450, 200):
        o = fr.oracle_on_frames(weights, n_out)
        st = o["stage"]
        ratio_margin, corner_margin = fr.margins(st)
        assert int(st["good"].sum()) == 292 and len(o["rows"]) == min(292, n_out)
        assert ratio_margin > 1e-3 and corner_margin > 1e-4, (ratio_margin, corner_margin)
        assert len(set(o["oct"].tolist())) == 2 and len(set(o["lev"].tolist())) == 5
        assert np.linalg.norm(o["ori_vec"], axis=1).min() > 0.05
    r = fr.foreign_frames(weights)[3].numpy()
    assert len(np.unique(r)) == len(r) and not np.all(np.diff(r) <= 0)           # distinct and unsorted
