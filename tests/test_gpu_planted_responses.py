"""Detector decisions on planted response pyramids (run with -m gpu on an MI355X).

Behind the Hessian response the detector is discrete logic (csrc/detect.hip): a wrong branch adds no float noise, it drops, duplicates or
reorders keypoints.  Images reach most of those branches by accident or not at all, so here both sides get the SAME hand-built response
pyramid through the RespNet slot (tests/_planted.py) on an all-zero image, and the kernels must return the oracle's rows: the same ids
in the same order, bit-equal responses, LAFs within 1e-4 px (the bar of test_edge_cases for detector-only frames; the summation order
of the centroid's small-map convolution is host-specific, so no bit equality there).  tests/test_planted_oracle.py shows on the CPU
that every construction reaches the branch it is named after.  The budget rule (more than N rows: response descending, then (octave,
level, pixel) ascending; otherwise (octave, level, pixel) order) is _planted.select_rows."""
import numpy as np
import pytest
import torch

import _planted as pl
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ROWS = {}


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return affnet_amd


def rows_of(case):
    """the oracle's keep-all rows of a case: computed once per module run, shared by every budget, never modified"""
    if case.name not in _ROWS:
        _ROWS[case.name] = pl.oracle_rows(case.H, case.W, case.plant, **case.kw)
    return _ROWS[case.name]


def detect(amd, case, N, raw_div=None):
    nlevels = case.kw.get("nlevels", 3)
    fn = pl.planted_fn(case.H, case.W, case.plant, pl.plan_of(case.H, case.W, nlevels)[1])
    det = amd.ScaleSpaceAffinePatchExtractor(mrSize=pl.MR, border=pl.BORDER, num_features=N, num_Baum_iters=0, RespNet=fn, **case.kw).to(DEV)
    if raw_div is not None:
        det.raw_div = raw_div
    x = torch.zeros(1, 1, case.H, case.W, device=DEV)
    runs = []
    for _ in range(2):
        r = det.run(x)                      # raises on a capacity overflow: a case that does not fit fails loudly, it is never truncated
        runs.append({k: r[k].cpu().clone() for k in ("ids", "responses", "LAFs")})
    for k in ("ids", "responses", "LAFs"):
        assert torch.equal(runs[0][k], runs[1][k]), "%s: two runs differ in %s" % (case.name, k)
    return runs[0]


def check(amd, case, N, raw_div=None):
    want = pl.select_rows(rows_of(case), N)
    got = detect(amd, case, N, raw_div)
    ids, resp, lafs = got["ids"].numpy().astype(np.int64), got["responses"].numpy(), got["LAFs"].numpy()
    tag = "planted: %s, N = %d" % (case.name, N)
    assert ids.shape == want["ids"].shape, "%s: %d rows, the oracle has %d" % (tag, len(ids), len(want["ids"]))
    bad = np.nonzero((ids != want["ids"]).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first at row %d: got %s want %s" % (tag, bad.size, bad[0], ids[bad[0]], want["ids"][bad[0]])
    assert np.array_equal(resp.view(np.uint32), want["resp"].view(np.uint32)), "%s: responses are not bit-equal" % tag
    err = float(np.abs(lafs - want["lafs"]).max())
    print("%s: %d rows, LAF max %.3g px" % (tag, len(ids), err))
    record_parity(tag, keypoints=int(len(ids)), laf_max_px=err)
    assert err < 1e-4, "%s: LAFs differ by %.3g px" % (tag, err)
    return want


def keep_all(case):
    return len(rows_of(case)["resp"]) + 100


# ---- hessian_nms_kernel: tile seams, partial tiles, the staging list -----------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(70, 131), (33, 65), (16, 64), (17, 193)], ids=lambda s: "%dx%d" % s)
def test_planted_tile_seams_and_partial_tiles(amd, hw):
    """Maxima on both sides of every 64-column / 16-row seam, in partial tiles and in every octave (16 x 64 and 17 x 193: a single octave).
    The default raw-maxima lists hold every size (the fullest: 1098 of 2292 entries in octave 0 of 70 x 131)."""
    case = pl.seams(*hw)
    check(amd, case, keep_all(case))


@pytest.mark.parametrize("N", ["all", 1000])
def test_planted_dense_tiles_overflow_the_staging_list(amd, N):
    """More than HN_CAP = 320 maxima in every 64 x 16 tile: the entries behind the staging list are appended one by one.  raw_div = 2: the
    2242 raw maxima of octave 0 (6144 pixels) do not fit the default list of h w / 4 = 1536 entries - with the default the existing overflow
    error must surface, never a truncated result."""
    case = pl.dense_tiles()
    if N == "all":
        with pytest.raises(amd._lib.AffnetHipError, match="overflow"):
            detect(amd, case, keep_all(case))
    check(amd, case, keep_all(case) if N == "all" else N, raw_div=2)


# ---- octaveMap replay: two-launch resolve (nlevels = 3) and the sequential level_resolve_kernel (nlevels >= 4) -----------------------------
@pytest.mark.parametrize("nlevels", [3, 4, 6])
@pytest.mark.parametrize("v", pl.STACK_VALUES)
def test_planted_stack(amd, v, nlevels):
    """One pixel, one value in pyramid levels 1, 2, 3: the slack keeps all three maxima, the uint8 octaveMap (wrap included) decides what is
    left: rows at every level (0.75), the first only (1.5), a negative row that resets the map (2.5), two wrapped negative rows (300.25).
    nlevels = 6: eight levels per octave, the largest instantiation of the NMS kernel."""
    case = pl.stack(v, nlevels)
    want = check(amd, case, keep_all(case))
    at = want["ids"][:, 2] == pl.STACK_PIXEL[0] * case.W + pl.STACK_PIXEL[1]
    assert [(int(l), float(r)) for l, r in zip(want["ids"][at, 1], want["resp"][at])] == pl.STACK_ROWS[v]


@pytest.mark.parametrize("nlevels", [3, 4])
@pytest.mark.parametrize("name", ["wrap_table", "slack", "skip_rule"])
def test_planted_replay_rules(amd, name, nlevels):
    """wrap_table: float -> int64 -> uint8 of fourteen level-1 values under a level-3 maximum (absent exactly where the map becomes 1, negative
    where it becomes 2 or more); slack: the NMS's +1e-5 on straight and diagonal neighbours; skip_rule: a level with one positive maximum
    yields nothing and leaves the map alone, a level with two yields both."""
    case = getattr(pl, name)(nlevels)
    check(amd, case, keep_all(case))


# ---- select_prepare_kernel / select_compact_kernel / select_rank_kernel --------------------------------------------------------------------
@pytest.mark.parametrize("kind,hw,N", [("digit3", (384, 512), 3000), ("digit2", (384, 512), 3000), ("digit3", (192, 256), 2000)],
                         ids=["384x512-third-digit", "384x512-second-digit", "192x256-lds-list"])
def test_planted_single_first_digit_bucket(amd, kind, hw, N):
    """Every candidate in one first-digit bucket of the radix select: 20708 of them (more than SEL_LIST_CAP: the bucket is re-read from global
    memory) or 4920 (the LDS list); the second or the third digit decides alone, the cut falls inside a group of ties that the order keys
    split, and the rank sort meets equal responses across its 256-row chunks."""
    check(amd, pl.single_bucket(hw[0], hw[1], kind), N)


@pytest.mark.parametrize("N", [1, 1131, 1500, 2672])
def test_planted_all_equal_responses(amd, N):
    """One response value in two levels of each of two octaves: the 44-bit order keys alone decide who is inside the budget (1131 = exactly
    the first (octave, level) group, 2672 = all rows but the last)."""
    check(amd, pl.all_equal(), N)


def test_planted_many_first_digit_buckets(amd):
    check(amd, pl.wide_range(), 1500)


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_planted_budget_at_the_row_count(amd, d):
    """n - 1, n and n + 1: the switch between the top-C mode (response order) and keep-all ((octave, level, pixel) order) is `n > C`"""
    case = pl.one_lattice()
    check(amd, case, len(rows_of(case)["resp"]) + d)


def test_planted_threshold_mode(amd):
    """th = 3.3: a response equal to the threshold clamps to zero and is no candidate, the next float above it is one (2.4e-7)"""
    case = pl.threshold_mode()
    want = check(amd, case, -1)
    assert len(want["resp"]) == 8 and float(want["resp"].min()) < 1e-6
