"""Unit sweep of csrc/handcrafted.hip - hc19_kernel<0> (orientation) and hc19_kernel<1> (Baumberg), the slots a default-constructed
ScaleSpaceAffinePatchExtractor runs - against the float64 restatements of tests/_handcrafted_fp64.py on ramps through every histogram
bin, noise, blobs, constant patches and the golden patches; at patch counts around the 64-lane edge; and through the pyramid entry
point affnet_handcrafted_forward_pyr (count, batch, id clamping, its own bilinear sampling).  tests/test_handcrafted_host.py checks
on the CPU that the fixture meets the conditions this module relies on.

Equal maxima are NOT covered.  The wave argmax ("first maximum wins") decides between two exactly equal smoothed bins only if two bins
receive bit-identical sums in the float64 restatement AND in the kernel's fp32.  Every pixel feeds one bin with (1 - frac(o_big)) * mag *
window: a mirrored or rotated copy of a gradient field lands in another bin with frac -> 1 - frac (mirror) or with o_big shifted by a
multiple of 9 that neither arithmetic reproduces exactly (rotation), and the one direction whose o_big is exact in both arithmetics -
atan2(0, g > 0) = 0, o_big = 18 - feeds a single bin.  No patch was found whose tie survives both roundings, so the case is left out; the
constant patches (one bin alone, its two neighbours exactly equal after smoothing) still pin that the maximum itself is found."""
import numpy as np
import pytest
import torch

import _handcrafted_fp64 as hc
import affnet_oracle as orc
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0
COUNTS = [1, 2, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return affnet_amd


@pytest.fixture(scope="module")
def fam():
    patches, names, family = hc.families()
    return {"patches": patches, "names": names, "family": family, "ori": hc.orientation_f64(patches), "dev": torch.from_numpy(patches).to(DEV)}


def _st():
    from affnet_amd import engine
    return engine.stream_of(torch.device(DEV))


def _forward(kind, patches, n, window, rows=None, angles=True):
    """affnet_handcrafted_forward on the first n patches into buffers of `rows` (default n + 1) sentinel rows."""
    from affnet_amd import engine
    from affnet_amd._lib import lib, check, ptr
    rows = n + 1 if rows is None else rows
    out = torch.full((rows, 2, 2), SENTINEL, device=DEV)
    ang = torch.full((rows,), SENTINEL, device=DEV) if angles else None
    ctx = engine.utility_ctx(torch.device(DEV))
    win = torch.from_numpy(np.ascontiguousarray(window, dtype=np.float32).reshape(-1))          # a host table
    check(lib.affnet_handcrafted_forward(ctx, kind, ptr(patches), n, ptr(win), ptr(out), ptr(ang), _st()), ctx, "affnet_handcrafted_forward")
    torch.cuda.synchronize()
    return out, ang


@pytest.fixture(scope="module")
def full(amd, fam):
    """Both kinds on all patches through the C entry point, with the oracle's fp32 windows."""
    n = fam["dev"].size(0)
    R, ang = _forward(0, fam["dev"], n, hc.orientation_window())
    A, _ = _forward(1, fam["dev"], n, hc.baumberg_window(), angles=False)
    return {"R": R, "ang": ang, "A": A}


# ---- orientation ---------------------------------------------------------------------------------------------------------------------------
def _check_orientation(tag, ang, R, fam):
    r, names = fam["ori"], fam["names"]
    ang, R = ang.cpu().numpy(), R.cpu().numpy()
    bins = hc.bin_of_angle(ang)
    dec = r["decided"]
    # the angle is exactly the kernel's expression of an integer bin
    want_ang = -(((np.float32(hc.TWO_PI32) * bins.astype(np.float32)) / np.float32(36.0)) - np.float32(hc.PI32))
    assert np.abs(ang - want_ang).max() < 1e-6, tag
    wrong = [(names[i], int(bins[i]), int(r["bin"][i])) for i in np.nonzero(dec & (bins != r["bin"]))[0]]
    stray = [(names[i], int(bins[i]), r["top2"][i].tolist()) for i in np.nonzero(~dec & (bins != r["top2"][:, 0]) & (bins != r["top2"][:, 1]))[0]]
    covered = sorted(set(bins[dec].tolist()))
    record_parity("hand-crafted orientation on the device: " + tag, patches=int(len(bins)), undecided=int((~dec).sum()), bins_covered=len(covered),
                  decided_wrong=len(wrong), undecided_outside_top2=len(stray), undecided_equal_to_restatement=int((bins[~dec] == r["bin"][~dec]).sum()))
    print("%s: %d patches, %d undecided, %d bins covered by decided patches, wrong %s, stray %s" % (tag, len(bins), (~dec).sum(), len(covered), wrong, stray))
    assert not wrong, "%s: decided patches in another bin (name, device, restatement): %s" % (tag, wrong)
    assert not stray, "%s: undecided patches outside the restatement's two largest bins: %s" % (tag, stray)
    assert covered == list(range(36))
    want_R = np.stack([np.stack([np.cos(ang), np.sin(ang)], 1), np.stack([-np.sin(ang), np.cos(ang)], 1)], 1)
    assert np.abs(R - want_R).max() < 1e-6, tag
    assert np.array_equal(R[:, 0, 0], R[:, 1, 1]) and np.array_equal(R[:, 0, 1], -R[:, 1, 0])


def test_orientation_c_entry_point(amd, fam, full):
    n = fam["dev"].size(0)
    assert float(full["ang"][n]) == SENTINEL and bool((full["R"][n] == SENTINEL).all())
    _check_orientation("C entry point", full["ang"][:n], full["R"][:n], fam)


def test_orientation_module(amd, fam, full):
    from affnet_amd.HandCraftedModules import OrientationDetector
    det = OrientationDetector(patch_size=19)
    ang = det(fam["dev"])
    R = det(fam["dev"], return_rot_matrix=True)
    _check_orientation("OrientationDetector(19)", ang, R, fam)
    # the module's window is the float64 product rounded once, the reference's the fp32 product: at most an ulp apart per tap, so the
    # decided patches - whose margin is 1e-5 relative - get the same bin from either
    dec = torch.from_numpy(fam["ori"]["decided"]).to(DEV)
    n = fam["dev"].size(0)
    assert torch.equal(ang[dec], full["ang"][:n][dec])


# ---- Baumberg ------------------------------------------------------------------------------------------------------------------------------
def test_baumberg_against_the_float64_restatement(amd, fam, full):
    from affnet_amd.HandCraftedModules import AffineShapeEstimator
    family, names = fam["family"], fam["names"]
    e_ref, got32, want, eig = hc.baumberg_reference_error(fam["patches"], family)
    ok = hc.well_conditioned(eig)
    n = len(names)
    assert bool((full["A"][n] == SENTINEL).all())
    for tag, Adev in (("C entry point", full["A"][:n]), ("AffineShapeEstimator(19)", AffineShapeEstimator(patch_size=19)(fam["dev"]))):
        A = Adev.cpu().numpy().astype(np.float64)
        figures = {}
        for f in "bce":
            sel = (family == f) & ok
            err = np.abs(A[sel] - want[sel]).reshape(int(sel.sum()), -1).max(axis=1)
            figures["err_" + f], figures["bar_" + f], figures["patches_" + f] = float(err.max()), 8.0 * e_ref[f][0], int(sel.sum())
            print("Baumberg %s, family %s: %d patches, worst |device - float64| %.3g, reference's own %.3g, bar %.3g" %
                  (tag, f, sel.sum(), err.max(), e_ref[f][0], 8.0 * e_ref[f][0]))
        record_parity("hand-crafted Baumberg on the device: " + tag, **figures)
        for f in "bce":
            assert figures["err_" + f] <= figures["bar_" + f], (tag, f, figures)
            assert np.all(A[(family == f) & ok][:, 0, 1] == 0.0)
        # ramps: rank-1 moment matrices - only the shape of the output: where a row is finite, up is up
        ramp = A[family == "a"]
        fin = np.isfinite(ramp).all(axis=(1, 2))
        assert np.all(ramp[fin][:, 0, 1] == 0.0), tag
        # constant patches: non-finite in the reference, and on the device in all four entries
        assert not np.isfinite(got32[family == "d"]).all(axis=(1, 2)).any()
        assert not np.isfinite(A[family == "d"]).any(), (tag, A[family == "d"])


# ---- patch counts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_patch_counts_leave_the_next_row_alone(amd, fam, full, n):
    R, ang = _forward(0, fam["dev"], n, hc.orientation_window())
    A, _ = _forward(1, fam["dev"], n, hc.baumberg_window(), angles=False)
    assert R.size(0) == n + 1
    # (NaN rows of the constant patches: compared as bits)
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert same(R[:n], full["R"][:n]) and same(ang[:n], full["ang"][:n]) and same(A[:n], full["A"][:n])
    assert bool((R[n] == SENTINEL).all()) and float(ang[n]) == SENTINEL and bool((A[n] == SENTINEL).all())


# ---- the pyramid entry point -----------------------------------------------------------------------------------------------------------------
def test_pyramid_entry_point_equals_sampled_patches(amd):
    """affnet_handcrafted_forward_pyr = affnet_handcrafted_forward on the patches affnet_pyr_grid_sample(ps = 19) writes for the same rows,
    bit for bit (both use aff_sample_bilinear and the same base grid); rows at or past the count keep what they held."""
    from affnet_amd._lib import lib, check, ptr
    xb = torch.cat([orc.synthetic_image(64, 80, s) for s in (1, 2, 3)], 0).to(DEV)
    det = amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=200, border=5, num_Baum_iters=0).to(DEV)
    det.enqueue(xb)
    torch.cuda.synchronize()
    ctx = det._ctx
    B, P = ctx.batch, ctx.cap_pre
    assert B == 3 and ctx.cfg.n_octaves >= 2
    resp = torch.empty(B, P, device=DEV); lafs = torch.empty(B, P, 2, 3, device=DEV); ids = torch.empty(B, P, 3, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    check(lib.affnet_detected_list(ctx.handle, ptr(resp), ptr(lafs), ptr(ids), ptr(cnt), _st()), ctx.handle, "affnet_detected_list")
    torch.cuda.synchronize()
    found = cnt.cpu().tolist()
    assert min(found) >= 8, found
    counts = [0, 1, min(found[2], 65)]
    dcount = torch.tensor(counts, dtype=torch.int32, device=DEV)
    assert len(set(map(tuple, ids[2, :counts[2], :2].cpu().tolist()))) >= 2          # more than one pyramid level among the rows
    ids = ids.clone()
    ids[2, 1, 0] = -1                                                                # octave below the range: clamped to 0
    ids[2, 2, 0] = ctx.cfg.n_octaves                                                 # and above it: clamped to the last
    ids[2, 3, 1] = ctx.cfg.levels_per_octave + 3                                     # level above the range
    ids[2, 4, 1] = -7
    patches = torch.full((B, P, 19, 19), SENTINEL, device=DEV)
    check(lib.affnet_pyr_grid_sample(ctx.handle, ptr(lafs), ptr(ids), ptr(dcount), P, 19, ptr(patches), _st()), ctx.handle, "affnet_pyr_grid_sample")
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    for kind, window in ((0, hc.orientation_window()), (1, hc.baumberg_window())):
        win = torch.from_numpy(window.reshape(-1).copy())
        out = torch.full((B, P, 2, 2), SENTINEL, device=DEV)
        check(lib.affnet_handcrafted_forward_pyr(ctx.handle, kind, ptr(lafs), ptr(ids), ptr(dcount), P, ptr(win), ptr(out), _st()), ctx.handle,
              "affnet_handcrafted_forward_pyr")
        torch.cuda.synchronize()
        for b, c in enumerate(counts):
            assert bool((out[b, c:] == SENTINEL).all()), (kind, b)
            if c == 0:
                continue
            assert float(patches[b, :c].std()) > 1.0 and bool((patches[b, c:] == SENTINEL).all())
            want, _ = _forward(kind, patches[b, :c].contiguous(), c, window, angles=False)
            assert same(out[b, :c], want[:c]), (kind, b)
        if kind == 0:
            bins = hc.bin_of_angle(np.arctan2(out[2, :counts[2], 0, 1].cpu().numpy(), out[2, :counts[2], 0, 0].cpu().numpy()))
            assert len(set(bins.tolist())) >= 4                                      # real image content: several orientations
    record_parity("hand-crafted slots through the pyramid entry point", counts=counts, detected=found)
