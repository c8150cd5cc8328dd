"""CPU only: every planted construction of tests/_planted.py does, on the reference's restatement alone, what it is named after - so that
the GPU cases of tests/test_gpu_planted_responses.py cannot pass vacuously (a lattice that no longer fills a radix bucket, a tile that
stays under the staging capacity, a stack whose octaveMap never wraps).  The figures in the comments are what the oracle gives for
these builders; the assertions are the conditions a kernel branch needs."""
import os
import re

import numpy as np
import pytest

import _planted as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETECT = open(os.path.join(ROOT, "affnet_amd", "csrc", "detect.hip")).read()

_ROWS = {}


def rows_of(case):
    if case.name not in _ROWS:
        _ROWS[case.name] = pl.oracle_rows(case.H, case.W, case.plant, **case.kw)
    return _ROWS[case.name]


def radix_key(resp):
    """detect.hip order_key(): larger float -> larger uint32 (digits of the radix select: bits 31..21, 20..10, 9..0)"""
    u = np.ascontiguousarray(resp, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def constant(name):
    m = re.search(r"#define %s (\d+)\b" % name, DETECT)
    assert m, "%s is no longer a #define of detect.hip" % name
    return int(m.group(1))


def at_pixel(rows, W, y, x, octave=0):
    """[(detection level, response)] of the rows at one pixel"""
    sel = (rows["ids"][:, 0] == octave) & (rows["ids"][:, 2] == y * W + x)
    return [(int(l), float(r)) for l, r in zip(rows["ids"][sel, 1], rows["resp"][sel])]


def test_the_kernel_constants_the_cases_are_built_around():
    assert constant("HN_CAP") == 320 and constant("SEL_LIST_CAP") == 8192 and constant("HT_X") == 64 and constant("HT_Y") == 16


def test_planted_fn_does_not_depend_on_the_call_order():
    case = pl.all_equal()
    shapes, sigmas = pl.plan_of(case.H, case.W)
    fn = pl.planted_fn(case.H, case.W, case.plant, sigmas)
    import torch
    calls = [(o, l) for o in range(len(shapes)) for l in range(5)]
    for o, l in calls[::-1] + calls:
        got = fn(torch.zeros(1, 1, *shapes[o]), sigmas[o][l])
        want = case.plant.get((o, l))
        assert tuple(got.shape) == (1, 1) + shapes[o]
        assert (float(got.abs().sum()) == 0.0) if want is None else torch.equal(got, want)
    got[...] = 1.0                                           # a caller writing into the result must not change the plant
    assert float(fn(torch.zeros(1, 1, *shapes[-1]), sigmas[-1][4]).abs().sum()) == 0.0


def test_select_rows_is_the_stated_order():
    ids = np.array([[0, 0, 7], [0, 1, 3], [1, 0, 2], [0, 0, 9], [1, 1, 1]], dtype=np.int64)
    rows = {"ids": ids, "resp": np.array([2.0, 5.0, 2.0, 2.0, -1.0], dtype=np.float32), "lafs": np.zeros((5, 2, 3), np.float32)}
    assert pl.select_rows(rows, 3)["ids"].tolist() == [[0, 1, 3], [0, 0, 7], [0, 0, 9]]          # ties at the cut: key order
    assert pl.select_rows(rows, 4)["ids"].tolist() == [[0, 1, 3], [0, 0, 7], [0, 0, 9], [1, 0, 2]]
    for N in (5, 6, -1):                                                                         # not more than N rows: key order
        assert pl.select_rows(rows, N)["ids"].tolist() == [[0, 0, 7], [0, 0, 9], [0, 1, 3], [1, 0, 2], [1, 1, 1]]


def test_single_bucket_needs_the_global_memory_pass_and_the_third_digit_alone():
    """384 x 512: 20708 candidates in ONE first-digit bucket (> SEL_LIST_CAP: in_lds == false), one value of key >> 10 (digits 1 and 2 decide
    nothing), and the cut at N = 3000 falls inside a group of ties."""
    rows = rows_of(pl.single_bucket(384, 512, "digit3"))
    k = radix_key(rows["resp"])
    n = len(k)
    want = pl.select_rows(rows, 3000)
    T = want["resp"][-1]
    ties, taken = int((rows["resp"] == T).sum()), int((want["resp"] == T).sum())
    print("candidates %d, distinct key>>21 %d, key>>10 %d, values %d, threshold tied %d, inside the cut %d"
          % (n, len(np.unique(k >> 21)), len(np.unique(k >> 10)), len(np.unique(k)), ties, taken))
    assert n == 20708 and n > constant("SEL_LIST_CAP")
    assert len(np.unique(k >> 21)) == 1 and len(np.unique(k >> 10)) == 1 and len(np.unique(k)) > 900
    assert ties > taken >= 1
    # equal responses on both sides of a 256-row chunk boundary of the rank sort
    r = want["resp"]
    assert any(r[i - 1] == r[i] for i in range(256, len(r), 256))


def test_single_bucket_with_many_second_digits():
    rows = rows_of(pl.single_bucket(384, 512, "digit2"))
    k = radix_key(rows["resp"])
    print("candidates %d, distinct key>>21 %d, key>>10 %d" % (len(k), len(np.unique(k >> 21)), len(np.unique(k >> 10))))
    assert len(k) > constant("SEL_LIST_CAP") and len(np.unique(k >> 21)) == 1 and len(np.unique(k >> 10)) > 1000


def test_small_single_bucket_stays_on_the_lds_list_path():
    rows = rows_of(pl.single_bucket(192, 256, "digit3"))
    k = radix_key(rows["resp"])
    assert len(k) == 4920 and 2000 < len(k) <= constant("SEL_LIST_CAP") and len(np.unique(k >> 10)) == 1
    T = pl.select_rows(rows, 2000)["resp"][-1]
    assert int((rows["resp"] == T).sum()) > int((pl.select_rows(rows, 2000)["resp"] == T).sum()) >= 1


def test_dense_tiles_overflow_the_staging_list_of_every_tile():
    case = pl.dense_tiles()
    rows = rows_of(case)
    ids = rows["ids"]
    assert len(ids) == 2242 and (ids[:, 0] == 0).all()
    tile_h, tile_w = constant("HT_Y"), constant("HT_X")
    ty, tx = (ids[:, 2] // case.W) // tile_h, (ids[:, 2] % case.W) // tile_w
    per_tile = [int(((ty == a) & (tx == b)).sum()) for a in range(-(-case.H // tile_h)) for b in range(-(-case.W // tile_w))]
    print("rows %d, per %dx%d tile %s" % (len(ids), tile_w, tile_h, per_tile))
    assert sum(per_tile) == len(ids) and min(per_tile) > constant("HN_CAP")
    assert sorted(set(ids[:, 1].tolist())) == [0, 2]


def test_all_equal_spans_octaves_and_levels():
    rows = rows_of(pl.all_equal())
    groups = {}
    for o, l in rows["ids"][:, :2].tolist():
        groups[(o, l)] = groups.get((o, l), 0) + 1
    print("rows %d, groups %s" % (len(rows["resp"]), groups))
    assert len(np.unique(rows["resp"])) == 1 and float(rows["resp"][0]) == 700.0
    assert len(groups) >= 3 and len({o for o, _ in groups}) == 2
    assert len(rows["resp"]) == 2673 and groups[(0, 0)] == 1131        # the budgets of the GPU case sit around these


@pytest.mark.parametrize("nlevels", [3, 4, 6])
@pytest.mark.parametrize("v", pl.STACK_VALUES)
def test_stack_pins_the_wrap_the_negative_rows_and_the_slack(v, nlevels):
    case = pl.stack(v, nlevels)
    got = at_pixel(rows_of(case), case.W, *pl.STACK_PIXEL)
    assert got == pl.STACK_ROWS[v], got
    assert len(rows_of(case)["resp"]) == len(got) + 2 * nlevels          # + the ballast, untouched


@pytest.mark.parametrize("nlevels", [3, 4])
def test_wrap_table(nlevels):
    case = pl.wrap_table(nlevels)
    rows = rows_of(case)
    for i, v in enumerate(pl.WRAP_VALUES):
        got = at_pixel(rows, case.W, pl.WRAP_ROW, pl.WRAP_X0 + 4 * i)
        m = float(np.uint8(np.int64(np.float32(v))))                      # octaveMap after level 1
        top = float(np.float32(pl.WRAP_TOP) * (np.float32(1.0) - np.float32(m)))
        want = [(0, float(np.float32(v)))] + ([(2, top)] if top != 0.0 else [])
        assert got == want, (v, got, want)
        assert (len(got) == 1) == (v in pl.WRAP_ABSENT), v
    assert any(r < 0 for r in rows["resp"])                               # 2.0, 3.7, 255.9, 511.9: negative rows are kept


@pytest.mark.parametrize("nlevels", [3, 4])
def test_slack(nlevels):
    case = pl.slack(nlevels)
    rows, P = rows_of(case), pl.SLACK_PIXELS
    assert pl.SLACK_NEAR > 5.0 and pl.SLACK_NEAR - 5.0 < 1e-5 < pl.SLACK_FAR - 5.0
    assert at_pixel(rows, case.W, *P["near_lo"]) == [(1, 5.0)] and at_pixel(rows, case.W, *P["near_hi"]) == [(1, pl.SLACK_NEAR)]
    assert at_pixel(rows, case.W, *P["far_lo"]) == [] and at_pixel(rows, case.W, *P["far_hi"]) == [(1, pl.SLACK_FAR)]


@pytest.mark.parametrize("nlevels", [3, 4])
def test_skip_rule(nlevels):
    case = pl.skip_rule(nlevels)
    rows = rows_of(case)
    by_level = {l: int((rows["ids"][:, 1] == l).sum()) for l in range(nlevels)}
    assert by_level[0] == 0 and by_level[1] == 2, by_level
    assert at_pixel(rows, case.W, 20, 30) == [(1, 9.0)]                   # positive: the skipped level left the octaveMap alone


def test_seams_put_maxima_on_every_tile_edge():
    cols, rws = set(), set()
    for H, W in ((70, 131), (33, 65), (16, 64), (17, 193)):
        case = pl.seams(H, W)
        rows = rows_of(case)
        shapes, _ = pl.plan_of(H, W)
        assert len(shapes) == {70: 3, 33: 2, 16: 1, 17: 1}[H]
        o0 = rows["ids"][rows["ids"][:, 0] == 0]
        cols |= set((o0[:, 2] % W).tolist())
        rws |= set((o0[:, 2] // W).tolist())
        assert len(set(rows["ids"][:, 1].tolist())) == 3 and len(rows["resp"]) > 20
    assert {63, 64, 127, 128} <= cols and {15, 16, 31, 32, 47, 48, 63, 64} <= rws


def test_wide_range_and_one_lattice():
    k = radix_key(rows_of(pl.wide_range())["resp"])
    assert len(np.unique(k >> 21)) > 100 and len(k) == 4920
    n = len(rows_of(pl.one_lattice())["resp"])
    assert n > 256                                                       # more than one chunk of the rank sort


def test_threshold_case():
    case = pl.threshold_mode()
    rows = rows_of(case)
    got = {p[:2]: at_pixel(rows, case.W, p[0], p[1]) for p in pl.TH_POINTS}
    th = np.float32(pl.TH)
    assert got[(20, 30)] == [] and got[(20, 50)] == []
    assert got[(20, 70)] == [(1, float(np.float32(pl.TH_NEXT) - th))] and 0 < got[(20, 70)][0][1] < 1e-6
    assert got[(20, 90)] == [(1, float(np.float32(5.0) - th))]
    assert len(rows["resp"]) == 2 + 6
