#!/usr/bin/env python
"""Time of the HardTFeat descriptor stage on the MI355X, HIP events, median of RUNS runs after WARM warm-ups, the
forms alternating inside one process on the same frames of a B x 1024 x 768 synthetic batch with N keypoints per image:

    (a) affnet_tfeat_forward_pyr                         patches sampled from the pyramid inside the trunk kernel
    (b) affnet_pyr_grid_sample + affnet_tfeat_forward    patch tensor through HBM
    (c) HardTFeatNet.forward restated with torch ops     on the patch tensor of (b), CHUNK patches at a time: what a caller had before
    (d) affnet_cnn32_forward_pyr(HardNet)                the HardNet descriptor stage on the same frames, for scale (seeded weights)

    python tools/tfeat_timing.py [B [N [RUNS]]]          defaults 32, 2000, 10;  writes $OUT/tfeat_timing.json (OUT defaults to out/)

Weights: the trained fixtures tests/golden/tfeat_weights_*.npz.  Reports ms per call, the run-to-run spread (max - min) of every form,
achieved TFLOP/s of (a) on 12 605 696 FLOP per valid row against the 157.3 TFLOP/s fp32 matrix peak, and the per-kernel split of (a) between
trunk, head GEMM and finish kernel from torch.profiler's device times (under the profiler: a little longer than in the timed runs; for
figures to quote run this tool under `rocprofv3 --kernel-trace --stats` in a run of its own).  (a) == (b) bit for bit, (c) within 1e-5; the acceptance is
(c) - (a) > the larger spread of the two."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples", "graf_matching"))
import affnet_amd  # noqa: E402
from affnet_amd import _lib, engine  # noqa: E402
from affnet_amd._lib import lib, check, ptr  # noqa: E402
from match_graf import load_tfeat_state  # noqa: E402

WARM = 2
CHUNK = 8192            # patches per torch-ops call: conv1's (CHUNK,32,26,26) output is 0.7 GB
FLOP_PER_PATCH = 12605696
PEAK_TFLOPS = 157.3


def torch_tfeat(x, sd):
    """(n,1,32,32) -> (n,128) with torch ops, step by step as HardTFeatNet.forward lists them."""
    flat = x.view(x.size(0), -1)
    mp, sp = flat.mean(1), flat.std(1) + 1e-7
    x = (x - mp.view(-1, 1, 1, 1)) / sp.view(-1, 1, 1, 1)
    x = F.max_pool2d(torch.tanh(F.conv2d(x, sd["features.0.weight"], sd["features.0.bias"])), 2, 2)
    x = torch.tanh(F.conv2d(x, sd["features.3.weight"], sd["features.3.bias"]))
    x = torch.tanh(F.conv2d(x, sd["classifier.1.weight"], sd["classifier.1.bias"])).view(x.size(0), -1)
    return x / torch.sqrt((x * x).sum(1, keepdim=True) + 1e-8)


def main(argv):
    B = int(argv[0]) if len(argv) > 0 else 32
    N = int(argv[1]) if len(argv) > 1 else 2000
    runs = int(argv[2]) if len(argv) > 2 else 10
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    ld = lambda k: torch.load(os.path.join(ROOT, "pretrained", k + ".pth"), map_location="cpu", weights_only=False)["state_dict"]
    A = affnet_amd.AffNetFast(PS=32); A.load_state_dict(ld("AffNet"))
    O = affnet_amd.OriNetFast(PS=32); O.load_state_dict(ld("OriNet"))
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=N, border=5, num_Baum_iters=1, AffNet=A.to(dev), OriNet=O.to(dev)).to(dev)
    net = affnet_amd.HardTFeatNet(sm=None)
    net.load_state_dict(load_tfeat_state(None))
    net = net.to(dev)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    hard = affnet_amd.HardNet(); hard.load_state_dict(affnet_amd.synthetic_hardnet_state(0)); hard = hard.to(dev)
    x = torch.cat([affnet_amd.synthetic_image(768, 1024, s) for s in range(B)], 0).to(dev)
    r = det.enqueue(x, do_ori=True)
    ctx, st = det._ctx, engine.stream_of(dev)
    ctx.read_counts()
    Fc = ctx.cap_final
    lafs, count = r["LAFs"].view(B, Fc, 2, 3), r["count"]
    lvl = torch.empty(B, Fc, 3, dtype=torch.int32, device=dev)
    norm = torch.empty(B, Fc, 2, 3, dtype=torch.float32, device=dev)
    check(lib.affnet_level_select(ctx.handle, ptr(lafs), ptr(count), Fc, 32, ptr(lvl), ptr(norm), st), ctx.handle, "affnet_level_select")
    packed, hpacked = net.packed_weights(dev), hard.packed_weights(dev)
    scratch = torch.empty(lib.affnet_tfeat_scratch_floats(B * Fc), dtype=torch.float32, device=dev)
    hscratch = torch.empty(B * Fc * (8192 + 512), dtype=torch.float32, device=dev)
    d_a = torch.zeros(B, Fc, 128, dtype=torch.float32, device=dev)
    d_b = torch.zeros(B * Fc, 128, dtype=torch.float32, device=dev)
    d_c = torch.zeros(B * Fc, 128, dtype=torch.float32, device=dev)
    d_h = torch.zeros(B, Fc, 128, dtype=torch.float32, device=dev)
    patches = torch.zeros(B * Fc, 1, 32, 32, dtype=torch.float32, device=dev)
    util = engine.utility_ctx(dev)

    def form_a():
        check(lib.affnet_tfeat_forward_pyr(ctx.handle, ptr(packed), ptr(norm), ptr(lvl), ptr(count), Fc, ptr(d_a), ptr(scratch), st), ctx.handle, "tfeat_forward_pyr")

    def form_b():
        check(lib.affnet_pyr_grid_sample(ctx.handle, ptr(norm), ptr(lvl), ptr(count), Fc, 32, ptr(patches), st), ctx.handle, "pyr_grid_sample")
        check(lib.affnet_tfeat_forward(util, ptr(packed), ptr(patches), None, B * Fc, ptr(d_b), ptr(scratch), st), util, "tfeat_forward")

    def form_c():
        with torch.no_grad():
            for s in range(0, B * Fc, CHUNK):
                d_c[s:s + CHUNK] = torch_tfeat(patches[s:s + CHUNK], sd)

    def form_d():
        check(lib.affnet_cnn32_forward_pyr(ctx.handle, _lib.NET_HARDNET, ptr(hpacked), ptr(norm), ptr(lvl), ptr(count), Fc, ptr(d_h), ptr(hscratch), st),
              ctx.handle, "cnn32_forward_pyr")

    forms = (("a_tfeat_forward_pyr", form_a), ("b_grid_sample_plus_tfeat_forward", form_b), ("c_torch_ops_on_patches", form_c),
             ("d_hardnet_forward_pyr", form_d))
    times = {k: [] for k, _ in forms}
    for it in range(WARM + runs):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= WARM:
                times[name].append(e0.elapsed_time(e1))
    rows = count.cpu().numpy()
    valid = (torch.arange(Fc, device=dev)[None, :] < count[:, None].long()).view(-1)
    same_ab = bool(torch.equal(d_a.view(-1, 128)[valid], d_b[valid]))
    diff_c = float((d_c[valid] - d_a.view(-1, 128)[valid]).abs().max())
    doc = {"what": "HardTFeat descriptor stage, ms per call: median (min .. max) of %d runs after %d warm-ups, HIP events" % (runs, WARM),
           "command": "python tools/tfeat_timing.py %d %d %d" % (B, N, runs), "device": torch.cuda.get_device_name(0),
           "batch": B, "image": "1024x768 synthetic", "keypoints_per_image": N, "rows": int(rows.sum()),
           "a_equals_b_bit_for_bit": same_ab, "c_max_abs_diff_from_a": diff_c}
    for name, _ in forms:
        t = np.array(times[name])
        doc[name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "spread_ms": float(t.max() - t.min())}
    ta, tc = doc["a_tfeat_forward_pyr"], doc["c_torch_ops_on_patches"]
    doc["a_tflops"] = float(rows.sum()) * FLOP_PER_PATCH / (ta["median_ms"] * 1e-3) / 1e12
    doc["a_fraction_of_fp32_matrix_peak"] = doc["a_tflops"] / PEAK_TFLOPS
    doc["torch_minus_native_ms"] = tc["median_ms"] - ta["median_ms"]
    doc["native_beats_torch_by_more_than_the_spread"] = bool(doc["torch_minus_native_ms"] > max(ta["spread_ms"], tc["spread_ms"]))
    try:                       # per-kernel device times of form (a), taken UNDER the in-process profiler: it stretches the kernels, so the split
                               # does not sum to the event time above (figures to quote: a kernel trace of this tool in a run of its own)
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                form_a()
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            for tag in ("tfeat_trunk_kernel", "tfeat_head_kernel", "tfeat_finish_kernel"):
                if tag in ev.key:
                    total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    split[tag + "_ms"] = float(total) / max(1, ev.count) * 1e-3
        doc["a_kernel_split_under_profiler"] = split or None
    except Exception as e:     # the figures above do not depend on the profiler
        doc["a_kernel_split_under_profiler"] = "profiler unavailable: %s" % e
    out_dir = os.environ.get("OUT") or os.path.join(ROOT, "out")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(doc, open(os.path.join(out_dir, "tfeat_timing.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, indent=1, sort_keys=True))
    assert same_ab and diff_c < 1e-5, (same_ab, diff_c)
    assert doc["native_beats_torch_by_more_than_the_spread"], doc


if __name__ == "__main__":
    main(sys.argv[1:])
