"""The ledger of the workspace (affnet_probe_workspace_areas: the table affnet_ctx_create and affnet_bind_workspace carve the workspace from) on the
CPU: contexts bound to a 256-byte aligned HOST buffer, no kernel runs.  The areas must tile the workspace, agree with every offset the library
publishes, have the sizes DESIGN.md section 3 states, and each be described in that section's table; and the three images of
tests/test_gpu_workspace_state.py must meet their conditions under the oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _workspace_state as ws
from affnet_amd import _lib
from affnet_amd._lib import lib
from affnet_amd.host_plan import PyramidPlan

# (label, height, width, num_features, num_prefilter, batch, onepass, nlevels, border)
CASES = [("b1", 240, 320, 300, 450, 1, False, 3, 5), ("b3", 240, 320, 300, 450, 3, False, 3, 5),
         ("onepass_b1", 240, 320, 300, 300, 1, True, 3, 15), ("onepass_b3", 240, 320, 300, 300, 3, True, 3, 15),
         ("nlevels4", 240, 320, 300, 450, 1, False, 4, 5), ("nlevels4_b3", 240, 320, 300, 450, 3, False, 4, 5),
         ("odd", 241, 323, 300, 450, 1, False, 3, 5), ("odd_b3", 241, 323, 300, 450, 3, False, 3, 5)]


@pytest.fixture(scope="module")
def probes():
    return ws.load_probes()


def test_onepass_contexts_have_one_capacity():
    """Why the OnePassSIR cases above run 300 / 300 and not 300 / 450 like the plain ones: affnet_ctx_create refuses a OnePassSIR config whose prefilter
    differs from its feature budget (there is no per-patch shape stage to cut in), so P == F in every OnePassSIR context that can exist and the sizes of
    its extra areas cannot tell the two apart.  The plain cases (P = 450 B, F = 300 B) are the ones that do."""
    plan = PyramidPlan(240, 320, 3, 1.6, 15)
    cfg = plan.fill_config(ws.MR_SIZE, 0.0, 300, 450, batch=1, baum_iters=0, onepass=True)
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, C.byref(cfg)) == _lib.ERR_INVALID
    assert b"num_prefilter must equal num_features" in lib.affnet_last_error(h)
    assert lib.affnet_workspace_bytes(h) == 0
    lib.affnet_ctx_destroy(h)


class HostCtx(object):
    """A context of the product library bound to host memory (affnet_bind_workspace takes any 256-byte aligned buffer: nothing is launched here)"""

    def __init__(self, h, w, nf, npre, batch, onepass, nlevels, border):
        self.plan = PyramidPlan(h, w, nlevels, 1.6, border)
        cfg = self.plan.fill_config(ws.MR_SIZE, 0.0, nf, npre, batch=batch, baum_iters=0 if onepass else 1, onepass=onepass)
        self.handle = C.c_void_p()
        assert lib.affnet_ctx_create(C.byref(self.handle), 0, C.byref(cfg)) == 0, lib.affnet_last_error(self.handle)
        self.bytes = int(lib.affnet_workspace_bytes(self.handle))
        self.mem = np.zeros(self.bytes + ws.ALIGN, dtype=np.uint8)
        self.base = (self.mem.ctypes.data + ws.ALIGN - 1) // ws.ALIGN * ws.ALIGN
        assert lib.affnet_bind_workspace(self.handle, C.c_void_p(self.base), self.bytes) == 0, lib.affnet_last_error(self.handle)
        self.B, self.P, self.F = batch, lib.affnet_capacity_prefilter(self.handle), lib.affnet_capacity_final(self.handle)
        self.onepass, self.levels = onepass, self.plan.levels_per_octave

    def close(self):
        lib.affnet_ctx_destroy(self.handle)


@pytest.fixture(params=CASES, ids=[c[0] for c in CASES])
def hc(request):
    c = HostCtx(*request.param[1:])
    yield c
    c.close()


def _al(x, a=ws.ALIGN):
    return (x + a - 1) // a * a


def _by_name(areas):
    out = {a["name"]: a for a in areas}
    assert len(out) == len(areas), "area names repeat"
    return out


def _inside(area, byte_off, nbytes=4):
    return area["offset"] <= byte_off and byte_off + nbytes <= area["offset"] + area["bytes"]


def test_units_tile_the_workspace(probes, hc):
    areas = ws.ledger(probes, hc.handle)
    units = [a for a in areas if a["parent"] < 0]
    end = 0
    for a in units:
        assert a["offset"] % ws.ALIGN == 0, a
        assert a["bytes"] > 0, a
        assert a["offset"] == _al(end), "%s does not start at the aligned end of the unit before it: gap or overlap" % a["name"]
        end = a["offset"] + a["bytes"]
    assert _al(end) == hc.bytes == lib.affnet_workspace_bytes(hc.handle)
    # views: inside their unit, 4-byte aligned; the arrays of a list lie back to back from the unit's start and fill it
    for i, a in enumerate(areas):
        if a["parent"] < 0:
            assert (a["kind"] == "group") == any(v["parent"] == i for v in areas), a
            continue
        u = areas[a["parent"]]
        assert u["parent"] < 0 and u["kind"] == "group" and a["kind"] != "group", a
        assert a["offset"] % 4 == 0 and a["bytes"] > 0 and _inside(u, a["offset"], a["bytes"]), a
        assert a["cleared"] == u["cleared"], a
    for i, u in enumerate(areas):
        views = [v for v in areas if v["parent"] == i]
        if not views or u["name"] == "cnn_scratch":
            continue
        pos = u["offset"]
        for v in views:
            assert v["offset"] == pos, "%s: the views of a list unit lie back to back" % v["name"]
            pos += v["bytes"]
        assert pos == u["offset"] + u["bytes"], u
    # the CNN scratch is a union: every view starts inside it, the largest reaches its end
    i = [a["name"] for a in areas].index("cnn_scratch")
    views = [v for v in areas if v["parent"] == i]
    assert max(v["offset"] + v["bytes"] for v in views) == areas[i]["offset"] + areas[i]["bytes"]


def test_published_offsets_fall_on_their_areas(probes, hc):
    by = _by_name(ws.ledger(probes, hc.handle))
    # pyramid levels of every image
    stride = lib.affnet_pyramid_image_stride(hc.handle)
    for b in range(hc.B):
        for o, (h, w) in enumerate(hc.plan.sizes):
            for l in range(hc.levels):
                off = 4 * (b * stride + lib.affnet_pyramid_level_offset(hc.handle, o, l))
                assert _inside(by["pyramid"], off, 4 * h * w), (b, o, l)
    assert 4 * lib.affnet_pyramid_level_offset(hc.handle, 0, 0) == by["pyramid"]["offset"]
    # counters
    cs = lib.affnet_counter_stride(hc.handle)
    assert cs == ws.CNT_TOTAL and by["counters"]["bytes"] == hc.B * cs * 4
    for b in range(hc.B):
        for which in range(5):
            assert _inside(by["counters"], 4 * (lib.affnet_counter_offset(hc.handle, which) + b * cs))
    # dense affine maps of a OnePassSIR context
    if hc.onepass:
        astride = lib.affnet_affmap_image_stride(hc.handle)
        assert 4 * lib.affnet_affmap_offset(hc.handle, 0) == by["affmap"]["offset"]
        for b in range(hc.B):
            for o, (h, w) in enumerate(hc.plan.sizes):
                assert _inside(by["affmap"], 4 * (b * astride + lib.affnet_affmap_offset(hc.handle, o)), 16 * h * w), (b, o)
    else:
        assert lib.affnet_affmap_offset(hc.handle, 0) == -1 and "affmap" not in by
    # the read-back offsets of the shape pass
    out = (C.c_int64 * 3)()
    assert probes.affnet_probe_shape_offsets(hc.handle, C.byref(out)) == 0
    assert 4 * out[0] == by["shape_A"]["offset"]
    assert 4 * out[1] == by["cnn_scratch.aff_reeval_flags"]["offset"]
    assert 4 * out[2] == by["det.lafs"]["offset"]


def test_sizes_follow_from_the_capacities(probes, hc):
    """DESIGN.md section 3, restated: B images, P = B * capacity_prefilter candidate rows, F = B * capacity_final output rows, CC = B * raw capacity"""
    by = _by_name(ws.ledger(probes, hc.handle))
    B, P, F = hc.B, hc.B * hc.P, hc.B * hc.F
    sizes = hc.plan.sizes
    pyr = _al(sum(hc.levels * h * w for h, w in sizes) * 4)
    omap = _al(sum(_al(h * w, 16) for h, w in sizes))
    raw = sum(max(256, h * w // 4) for h, w in sizes)
    CC = B * raw
    want = {"pyramid": B * pyr, "octave_map": B * omap, "raw": CC * ws.RAWMAX_BYTES, "counters": B * ws.CNT_TOTAL * 4, "sel_hist": B * ws.SEL_HIST_BINS * 4,
            "cand": CC * 28, "cand.resp": CC * 4, "cand.syx": CC * 12, "cand.ids": CC * 12,
            "sel": P * 28, "sel.resp": P * 4, "sel.syx": P * 12, "sel.ids": P * 12,
            "det": P * 40, "det.resp": P * 4, "det.lafs": P * 24, "det.ids": P * 12,
            "shape_A": P * 16, "shape_iter": P * 40, "shape_iter.A2": P * 16, "shape_iter.lafs": P * 24,
            "shape_key_good": P * 8, "shape_key_good.key": P * 4, "shape_key_good.good": P * 4, "rank": P * 4, "det_count": B * 4,
            "lafs_shaped": F * 24, "ori_R": F * 16, "desc_frames": F * 36, "desc_frames.lafs_norm": F * 24, "desc_frames.lvl_ids": F * 12,
            "cnn_scratch": max(F * (8192 + 4 * 128), P * 144) * 4, "cnn_scratch.aff_partials": P * 32 * 4, "cnn_scratch.aff_reeval_flags": P * 4,
            "cnn_scratch.ori_partials": F * 144 * 4, "cnn_scratch.hard_conv5": F * 8192 * 4, "cnn_scratch.hard_head_partials": F * 512 * 4}
    if hc.onepass:
        h0, w0 = sizes[0]
        want.update({"affmap": B * sum(_al(16 * h * w) for h, w in sizes), "dense": B * lib.affnet_fullconv_scratch_bytes(h0, w0),
                     "cand2": CC * 28, "cand2.resp": CC * 4, "cand2.syx": CC * 12, "cand2.ids": CC * 12,
                     "lvltab": B * _lib.MAX_OCTAVES * _lib.MAX_LEVELS * 16})
    assert set(by) == set(want), sorted(set(by) ^ set(want))
    for name, nbytes in want.items():
        assert by[name]["bytes"] == nbytes, (name, by[name]["bytes"], nbytes)
    kinds = {"pyramid": "f32", "octave_map": "u8", "raw": "records", "counters": "i32", "sel_hist": "i32", "rank": "i32", "det_count": "i32", "shape_A": "f32",
             "lafs_shaped": "f32", "ori_R": "f32", "affmap": "f32", "dense": "f32", "lvltab": "i32", "cnn_scratch.aff_reeval_flags": "i32",
             "shape_key_good.good": "i32", "desc_frames.lvl_ids": "i32"}
    for name, a in by.items():
        k = kinds.get(name, "i32" if name.endswith(".ids") else ("group" if "." not in name else "f32"))
        assert a["kind"] == k, (name, a["kind"], k)
    # what the detector half clears itself: the counters, the histogram, the detection list, the rank accumulator - and the octaveMap where it exists in
    # memory.  (The table's flag and the detector's choice of replay are one predicate, aff_detect_two_pass in csrc/common.h; this is its restatement.  That the
    # clear really happens when the flag says so is the GPU file's business: its nlevels 4 variant runs behind stale and NaN states.)
    cleared = {"counters", "sel_hist", "det", "det.resp", "det.lafs", "det.ids", "rank"} | ({"octave_map"} if hc.levels - 2 > 3 else set())
    assert {n for n, a in by.items() if a["cleared"]} == cleared
    # the views where the library itself computes them from the capacities (csrc/debug.hip, csrc/cnn32.hip)
    assert by["cnn_scratch.hard_head_partials"]["offset"] == by["cnn_scratch"]["offset"] + F * 8192 * 4
    assert by["cnn_scratch.aff_reeval_flags"]["offset"] == by["cnn_scratch"]["offset"] + P * 32 * 4


def test_design_table_names_every_area(probes):
    """Every ledger name of a plain and of a OnePassSIR context has a row in the audit table of DESIGN.md section 3"""
    names = set()
    for case in (CASES[0], CASES[2]):
        c = HostCtx(*case[1:])
        names |= {a["name"] for a in ws.ledger(probes, c.handle)}
        c.close()
    text = open(os.path.join(ws.ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 3. Data layout in HBM"):text.index("## 4. Kernels, rooflines")]
    rows = set()
    for line in sec.splitlines():
        if line.startswith("| `"):                     # a table row: its first cell names one area or the views of one list
            rows |= set(re.findall(r"`([A-Za-z0-9_.]+)`", line.split("|")[1]))
    assert names <= rows, "areas without a row in DESIGN.md section 3: %s" % sorted(names - rows)
    assert rows <= names, "rows of DESIGN.md section 3 that name no area: %s" % sorted(rows - names)


def test_probe_refuses_what_it_cannot_describe(probes):
    assert probes.affnet_probe_workspace_areas(None, 0, None) < 0
    h = C.c_void_p()
    assert lib.affnet_ctx_create(C.byref(h), 0, None) == 0          # utility context: no workspace
    assert probes.affnet_probe_workspace_areas(h, 0, None) < 0
    lib.affnet_ctx_destroy(h)
    c = HostCtx(*CASES[0][1:])
    n = probes.affnet_probe_workspace_areas(c.handle, 0, None)
    buf = (_lib.WsArea * (n + 1))()
    buf[2].name = b"untouched"
    assert probes.affnet_probe_workspace_areas(c.handle, 2, C.cast(buf, C.c_void_p)) == n      # writes `max` records, returns the number there are
    assert buf[1].name == b"octave_map" and buf[2].name == b"untouched"
    assert probes.affnet_probe_workspace_areas(c.handle, 2, None) < 0
    c.close()


# ---- the three images of the GPU test, under the oracle alone --------------------------------------------------------------------------------------
def test_images_meet_their_conditions(weights):
    sd = weights["AffNet"]
    cand, first, surv, rows = ws.oracle_counts(ws.rich_image(), sd)
    print("rich: %d candidates, %d survivors in the first %d, %d in all, %d rows" % (cand, first, ws.LAZY_ROWS, surv, rows))
    assert cand == ws.N_PREFILTER, "rich must fill the candidate list"
    assert first >= ws.N_FEATURES and rows == ws.N_FEATURES, "rich must reach its N survivors inside the first lazy window"
    cand, first, surv, rows = ws.oracle_counts(ws.poor_image(), sd)
    print("poor: %d candidates, %d survivors in the first %d, %d in all, %d rows" % (cand, first, ws.LAZY_ROWS, surv, rows))
    assert 1 <= rows <= 75 and rows == surv, "poor must leave between 1 and 75 rows"
    assert cand < ws.N_PREFILTER and first < ws.N_FEATURES, "poor must need the second lazy pass and end every list below its capacity"
    flat = ws.flat_image()
    assert float(flat.min()) == float(flat.max())
    assert ws.oracle_counts(flat, sd) == (0, 0, 0, 0), "flat must have no detections"
    # busy (a prior state only): full lists, and the second lazy pass runs
    cand, first, surv, rows = ws.oracle_counts(ws.busy_image(), sd)
    assert cand == ws.N_PREFILTER and first < ws.N_FEATURES <= surv
