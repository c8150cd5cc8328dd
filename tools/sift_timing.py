#!/usr/bin/env python
"""Time of the SIFT descriptor stage on the MI355X, HIP events, median of RUNS runs after WARM warm-ups, the
three forms alternating inside one process on the same frames of a B x 1024 x 768 synthetic batch with N keypoints per image:

    (a) affnet_sift_forward_pyr                          patches sampled from the pyramid inside the kernel
    (b) affnet_pyr_grid_sample + affnet_sift_forward     patch tensor through HBM
    (c) SIFTNet.forward restated with torch ops          on the patch tensor of (b): what a caller had before the native module

    python tools/sift_timing.py [B [N [RUNS]]]           defaults 32, 2000, 20;  writes $OUT/sift_timing.json (OUT defaults to out/)

Every timed run is INNER back-to-back calls between two events (the kernels are ~0.1 ms: one call is too short a window); the figure
is per call.  (a), (b) and (c) must agree: (a) == (b) bit for bit, (c) within 1e-5."""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import affnet_amd  # noqa: E402
from affnet_amd import engine  # noqa: E402
from affnet_amd._lib import lib, check, ptr  # noqa: E402

WARM, INNER = 3, 10


def torch_sift(x, gk, pk, clipval=0.2):
    """(n,1,32,32) -> (n,128) with torch ops, step by step as SIFTNet.forward lists them."""
    kx = torch.tensor([[[[-1.0, 0.0, 1.0]]]], device=x.device)
    gx = F.conv2d(F.pad(x, (1, 1, 0, 0), "replicate"), kx)
    gy = F.conv2d(F.pad(x, (0, 0, 1, 1), "replicate"), kx.transpose(2, 3))
    mag = torch.sqrt(gx ** 2 + gy ** 2 + 1e-10)
    ori = torch.atan2(gy, gx + 1e-8)
    mag = mag * gk.expand_as(mag)
    o = (ori + 2.0 * math.pi) / (2.0 * math.pi) * 8.0
    b0 = torch.floor(o)
    w1 = o - b0
    b0 = b0 % 8
    b1 = (b0 + 1) % 8
    w0m, w1m = (1.0 - w1) * mag, w1 * mag
    bins = [F.conv2d((b0 == i).float() * w0m + (b1 == i).float() * w1m, pk, stride=6) for i in range(8)]
    d = torch.cat(bins, 1).view(x.size(0), -1)
    norm = lambda v: v / torch.sqrt(torch.abs((v * v).sum(1, keepdim=True)) + 1e-10)
    return norm(torch.clamp(norm(d), 0.0, clipval))


def main(argv):
    B = int(argv[0]) if len(argv) > 0 else 32
    N = int(argv[1]) if len(argv) > 1 else 2000
    runs = int(argv[2]) if len(argv) > 2 else 20
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    ld = lambda k: torch.load(os.path.join(ROOT, "pretrained", k + ".pth"), map_location="cpu", weights_only=False)["state_dict"]
    A = affnet_amd.AffNetFast(PS=32); A.load_state_dict(ld("AffNet"))
    O = affnet_amd.OriNetFast(PS=32); O.load_state_dict(ld("OriNet"))
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=N, border=5, num_Baum_iters=1, AffNet=A.to(dev), OriNet=O.to(dev)).to(dev)
    net = affnet_amd.SIFTNet(patch_size=32)
    x = torch.cat([affnet_amd.synthetic_image(768, 1024, s) for s in range(B)], 0).to(dev)
    r = det.enqueue(x, do_ori=True)
    ctx, st = det._ctx, engine.stream_of(dev)
    ctx.read_counts()
    Fc = ctx.cap_final
    lafs, count = r["LAFs"].view(B, Fc, 2, 3), r["count"]
    lvl = torch.empty(B, Fc, 3, dtype=torch.int32, device=dev)
    norm = torch.empty(B, Fc, 2, 3, dtype=torch.float32, device=dev)
    check(lib.affnet_level_select(ctx.handle, ptr(lafs), ptr(count), Fc, 32, ptr(lvl), ptr(norm), st), ctx.handle, "affnet_level_select")
    win, gk = net.window(dev), net.window(dev).view(1, 1, 32, 32)
    pk = torch.from_numpy(affnet_amd.pytorch_sift.getPoolingKernel(11).astype(np.float32)).view(1, 1, 11, 11).to(dev)
    d_a = torch.zeros(B, Fc, 128, dtype=torch.float32, device=dev)
    d_b = torch.zeros(B * Fc, 128, dtype=torch.float32, device=dev)
    patches = torch.zeros(B * Fc, 1, 32, 32, dtype=torch.float32, device=dev)
    util = engine.utility_ctx(dev)
    out_c = [None]

    def form_a():
        check(lib.affnet_sift_forward_pyr(ctx.handle, ptr(norm), ptr(lvl), ptr(count), Fc, ptr(win), 0.2, ptr(d_a), st), ctx.handle, "sift_forward_pyr")

    def form_b():
        check(lib.affnet_pyr_grid_sample(ctx.handle, ptr(norm), ptr(lvl), ptr(count), Fc, 32, ptr(patches), st), ctx.handle, "pyr_grid_sample")
        check(lib.affnet_sift_forward(util, ptr(patches), B * Fc, ptr(win), 0.2, ptr(d_b), st), util, "sift_forward")

    def form_c():
        with torch.no_grad():
            out_c[0] = torch_sift(patches, gk, pk)

    forms = (("a_sift_forward_pyr", form_a), ("b_grid_sample_plus_sift_forward", form_b), ("c_torch_ops_on_patches", form_c))
    times = {k: [] for k, _ in forms}
    for it in range(WARM + runs):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record()
            e1.synchronize()
            if it >= WARM:
                times[name].append(e0.elapsed_time(e1) / INNER)
    rows = count.cpu().numpy()
    valid = (torch.arange(Fc, device=dev)[None, :] < count[:, None].long()).view(-1)
    same_ab = bool(torch.equal(d_a.view(-1, 128)[valid], d_b[valid]))
    diff_c = float((out_c[0][valid] - d_a.view(-1, 128)[valid]).abs().max())
    doc = {"what": "SIFT descriptor stage, ms per call: median (min .. max) of %d runs of %d calls after %d warm-ups, HIP events" % (runs, INNER, WARM),
           "command": "python tools/sift_timing.py %d %d %d" % (B, N, runs), "device": torch.cuda.get_device_name(0),
           "batch": B, "image": "1024x768 synthetic", "keypoints_per_image": N, "rows": int(rows.sum()),
           "a_equals_b_bit_for_bit": same_ab, "c_max_abs_diff_from_a": diff_c}
    for name, _ in forms:
        t = np.array(times[name])
        doc[name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}
    out_dir = os.environ.get("OUT") or os.path.join(ROOT, "out")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(doc, open(os.path.join(out_dir, "sift_timing.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, indent=1, sort_keys=True))
    assert same_ab and diff_c < 1e-5, (same_ab, diff_c)


if __name__ == "__main__":
    main(sys.argv[1:])
