"""OnePassSIR detector decisions on planted responses AND planted affine maps (run with -m gpu on an MI355X).

The OnePassSIR branch of csrc/detect.hip - onepass_level_select_kernel, onepass_filter_kernel, onepass_adopt_count_kernel,
select_emit_onepass_kernel and the histogram-less select_top on the filtered list - is discrete logic: a wrong branch drops rows, keeps
wrong ones or reorders them, and a handful of wrong rows fits inside the bars of the image tests (tests/test_gpu_onepass.py).  Here both
sides get the SAME hand-built response pyramid and the SAME hand-built affine maps through the RespNet / AffNet slots
(tests/_planted_onepass.py) on constant images, and the kernels must return what _planted_onepass.select_rows_onepass makes of the
oracle's per-level rows: the same ids in the same order, bit-equal responses, frame centres within 1e-4 px (the bar of
tests/test_gpu_planted_responses.py for detector-only frames) and 2 x 2 entries within 1e-4 px x max(1, max |a_ij| of the row): they are
that isotropic frame times a_ij.  tests/test_planted_onepass_oracle.py shows on the CPU that every construction reaches its branch and
that the rule is the oracle's own answer; both files walk _planted_onepass.ALL_RUNS."""
import numpy as np
import pytest
import torch

import _planted_onepass as po
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("ids", "responses", "LAFs")


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return affnet_amd


def detector(amd, p, N, resp_fn, aff_fn):
    return amd.OnePassSIR(mrSize=po.MR, border=po.BORDER, num_features=N, num_Baum_iters=0, nlevels=p.case.kw.get("nlevels", 3),
                          RespNet=resp_fn, AffNet=aff_fn).to(DEV)


def max_a(p, ids):
    """max |a_ij| of the planted map at every row's (octave, pixel)"""
    return np.array([float(p.maps[o][0].reshape(4, -1)[:, pix].abs().max()) for o, _, pix in ids.tolist()])


def compare(tag, p, got, want):
    ids, resp, lafs = got["ids"].numpy().astype(np.int64), got["responses"].numpy(), got["LAFs"].numpy()
    assert ids.shape == want["ids"].shape, "%s: %d rows, the oracle's rule gives %d" % (tag, len(ids), len(want["ids"]))
    bad = np.nonzero((ids != want["ids"]).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first at row %d: got %s want %s" % (tag, bad.size, bad[0], ids[bad[0]], want["ids"][bad[0]])
    assert np.array_equal(resp.view(np.uint32), want["resp"].view(np.uint32)), "%s: responses are not bit-equal" % tag
    d = np.abs(lafs.astype(np.float64) - want["lafs"].astype(np.float64))
    centre = float(d[:, :, 2].max()) if len(ids) else 0.0
    rel = float((d[:, :, :2].reshape(len(ids), 4).max(axis=1) / np.maximum(1.0, max_a(p, ids))).max()) if len(ids) else 0.0
    print("%s: %d rows, centre max %.3g px, 2x2 max %.3g px per max(1, |a|)" % (tag, len(ids), centre, rel))
    record_parity(tag, keypoints=int(len(ids)), laf_centre_max_px=centre, laf_2x2_max_px_per_a=rel)
    assert centre < 1e-4, "%s: frame centres differ by %.3g px" % (tag, centre)
    assert rel < 1e-4, "%s: 2x2 entries differ by %.3g px x max(1, max|a|)" % (tag, rel)


def check(amd, label, p, N):
    resp_fn, aff_fn = po.slots(p)
    det = detector(amd, p, N, resp_fn, aff_fn)
    x = torch.zeros(1, 1, p.case.H, p.case.W, device=DEV)
    runs = []
    for _ in range(2):
        r = det.run(x, do_ori=False)        # raises on a capacity overflow: a case that does not fit fails loudly
        runs.append({k: r[k].cpu().clone() for k in KEYS})
    for k in KEYS:
        assert torch.equal(runs[0][k], runs[1][k]), "%s: two runs differ in %s" % (label, k)
    assert len(det.aff_maps) == len(p.maps)
    for o, m in enumerate(p.maps):          # the maps the detector read are the planted ones, bit for bit
        assert torch.equal(det.aff_maps[o].cpu(), m), "%s: affine map of octave %d" % (label, o)
    compare("planted onepass: %s, N = %d" % (label, N), p, runs[0], po.select_rows_onepass(po.rows_of(p), N))


SINGLE = [r for r in po.ALL_RUNS if not r[0].startswith("batch3")]
BATCH = [r for r in po.ALL_RUNS if r[0].startswith("batch3")]


@pytest.mark.parametrize("run", SINGLE, ids=[i for i, r in zip(po.RUN_IDS, po.ALL_RUNS) if not r[0].startswith("batch3")])
def test_planted_onepass(amd, run):
    """Both slots foreign (affnet_detect_image_onepass_responses with packed = NULL).  offdiag: plane and octave indexing of the emit;
    boundary: the four inequalities of the corner test, one of them through a12 alone and one through a21 alone; cut_switch: n_pos at
    N - 1, N, N + 1 with CNT_POS0 from each of its three producers; cut_counts_positives: the octaveMap's zeros and negative rows are not
    counted; cut_before_filter: nothing is promoted, the table is indexed (octave, level); radix: the first byte, the last byte, bucket 0,
    ties beyond / equal to the need, N = 1."""
    label, p, N, _ = run
    check(amd, label, p, N)


def test_planted_onepass_batch_of_three(amd):
    """enqueue() on the constant images 0, 1, 2: image 1 has another plant and other maps than images 0 and 2 (one level cut in image 0, not
    in image 1), so an index into another image's lvltab, affine map or second candidate list shows; every image against its own rows."""
    ps = [r[1] for r in BATCH]
    N = BATCH[0][2]
    fns = [po.slots(p) for p in ps]
    det = detector(amd, ps[0], N, po.by_image_value([f[0] for f in fns]), po.by_image_value([f[1] for f in fns]))
    c = ps[0].case
    x = torch.cat([torch.full((1, 1, c.H, c.W), float(b)) for b in range(3)]).to(DEV)
    outs = []
    for _ in range(2):
        r = det.enqueue(x, do_ori=False)
        torch.cuda.synchronize()
        det._ctx.read_counts()              # raises on a capacity overflow
        outs.append({k: r[k].cpu().clone() for k in KEYS + ("count",)})
    for k in KEYS + ("count",):
        assert torch.equal(outs[0][k], outs[1][k]), "batch3: two runs differ in %s" % k
    for b, p in enumerate(ps):
        for o, m in enumerate(p.maps):
            assert torch.equal(det._ctx.affmap_views(b)[o].cpu(), m), "batch3: affine map of image %d octave %d" % (b, o)
        n = int(outs[0]["count"][b])
        compare("planted onepass: batch3 image %d, N = %d" % (b, N), p, {k: outs[0][k][b, :n] for k in KEYS},
                po.select_rows_onepass(po.rows_of(p, float(b)), N))


def test_planted_responses_with_the_native_dense_affnet(amd, weights):
    """The one smoke case of the slot combination RespNet foreign + AffNet native (packed != NULL with a response pyramid).  The dense
    net's own accuracy is the business of tests/test_gpu_onepass.py (map within 5e-5 of the oracle's): here the oracle is handed the maps
    the device computed, so the detector behind them is held to the bars above."""
    p0 = po.cut_before_filter()
    c = p0.case
    FC = amd.AffNetFastFullConv()
    FC.load_state_dict(weights["AffNet"])
    FC = FC.to(DEV)
    det = detector(amd, p0, po.BEFORE_N, po.slots(p0)[0], FC)
    r = det.run(torch.zeros(1, 1, c.H, c.W, device=DEV), do_ori=False)
    maps = [m.cpu().clone() for m in det.aff_maps]
    for m in maps:
        assert torch.isfinite(m).all() and float(m[0, 1].abs().max()) == 0.0
    p = po.Planted(c, maps)
    compare("planted onepass: responses planted, native dense AffNet", p, {k: r[k].cpu() for k in KEYS},
            po.select_rows_onepass(po.level_rows(p), po.BEFORE_N))
