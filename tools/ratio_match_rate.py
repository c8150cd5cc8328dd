#!/usr/bin/env python3
"""Time of one ratio-test matching call (affnet_match_ratio: norms + forward tiles + merge [+ FGINN tiles + merge] [+ backward tiles + merge] +
selection) without a radius, with radius 10 px, and with radius 10 px plus the mutual check, at 2000 x 2000 and 500 x 500 descriptors, next to
affnet_match_snn on the same descriptors; and 32 pairs of 2000 x 2000 through affnet_match_ratio_many against the loop of 32 single calls.  All in
the same process on the same library build.

    python tools/ratio_match_rate.py [--calls 50] [--windows 7] [--pairs 32] [--out FILE]

Each figure is the time between two device events around `--calls` back-to-back calls on caller-owned buffers (no allocation, no read-back in the
window), divided by the number of calls (the many-pairs variants: --calls / 10 calls, each of all pairs); every variant is warmed up first, the
windows of all variants alternate, and median / min / max over the windows are reported, so the spread is visible next to the number.  Input: the
planted planar scene of tools/guided_rate.py, generated from a seed.  Also reported: the chunks the library chose and what each call kept.
Fails without a GPU.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from guided_rate import descriptors, planar_scene  # noqa: E402

INF = float("inf")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ratio_match_rate: no GPU - a time is measured on the device or not at all")
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device("cuda:0")
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    variants, chunks = {}, {}
    modes = (("snn", -1.0, 0), ("fginn", 10.0, 0), ("fginn_mutual", 10.0, 1))
    for T in (500, 2000):
        _, l2, tent = planar_scene(T, T)
        d1, d2 = descriptors(tent, T)
        D1, D2, L2 = (torch.from_numpy(a).to(dev) for a in (d1, d2, l2))
        dist = torch.zeros(T, 2, dtype=torch.float32, device=dev)
        idx = torch.zeros(T, 2, dtype=torch.int32, device=dev)
        tn = torch.zeros(T, 2, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.affnet_match_ratio_scratch_bytes(T, T, 0), dtype=torch.uint8, device=dev)
        keep = [D1, D2, L2, dist, idx, tn, scratch]
        chunks["T%d" % T] = int(lib.affnet_knn_chunks(ctx, T, T))
        for name, radius, flags in modes:
            def ratio(D1=D1, D2=D2, L2=L2, T=T, radius=radius, flags=flags, dist=dist, idx=idx, tn=tn, cnt=cnt, scratch=scratch):
                check(lib.affnet_match_ratio(ctx, ptr(D1), T, ptr(D2), T, 128, ptr(L2), radius, 0.8, INF, flags, 0, ptr(dist), ptr(idx), ptr(tn), ptr(cnt),
                                             ptr(scratch), st), ctx, "affnet_match_ratio")
            variants["ratio_%s_T%d" % (name, T)] = (ratio, cnt, keep, args.calls)
        md, md2 = torch.zeros(T, device=dev), torch.zeros(T, device=dev)
        mi = torch.zeros(T, dtype=torch.int32, device=dev)
        tn2 = torch.zeros(T, 2, dtype=torch.int32, device=dev)
        cnt2 = torch.zeros(1, dtype=torch.int32, device=dev)
        scratch2 = torch.empty(lib.affnet_match_scratch_bytes(T, T), dtype=torch.uint8, device=dev)

        def snn(D1=D1, D2=D2, T=T, md=md, mi=mi, md2=md2, tn2=tn2, cnt2=cnt2, scratch2=scratch2):
            check(lib.affnet_match_snn(ctx, ptr(D1), T, ptr(D2), T, 128, 0.8, ptr(md), ptr(mi), ptr(md2), ptr(tn2), ptr(cnt2), ptr(scratch2), st), ctx,
                  "affnet_match_snn")
        variants["match_snn_T%d" % T] = (snn, cnt2, keep + [md, md2, mi, tn2, scratch2], args.calls)
    # P pairs of 2000 x 2000: every pair its own images, back to back
    P, T = args.pairs, 2000
    sides = [(planar_scene(T, 100 + p), p) for p in range(P)]
    descs = [descriptors(s[2], 100 + p) for s, p in sides]
    A = torch.from_numpy(np.concatenate([d[0] for d in descs])).to(dev)
    B = torch.from_numpy(np.concatenate([d[1] for d in descs])).to(dev)
    LB = torch.from_numpy(np.concatenate([s[1] for s, _ in sides])).to(dev)
    table = torch.tensor([[p * T, T, p * T, T] for p in range(P)], dtype=torch.int32, device=dev)
    mdist = torch.zeros(P, T, 2, dtype=torch.float32, device=dev)
    midx = torch.zeros(P, T, 2, dtype=torch.int32, device=dev)
    mtn = torch.zeros(P, T, 2, dtype=torch.int32, device=dev)
    mcnt = torch.zeros(P, dtype=torch.int32, device=dev)
    mscratch = torch.empty(lib.affnet_match_ratio_many_scratch_bytes(P, T, T, 0), dtype=torch.uint8, device=dev)
    sscratch = torch.empty(lib.affnet_match_ratio_scratch_bytes(T, T, 0), dtype=torch.uint8, device=dev)
    keep = [A, B, LB, table, mdist, midx, mtn, mcnt, mscratch, sscratch]
    seg = [(ptr(A[p * T:]), ptr(B[p * T:]), ptr(LB[p * T:]), ptr(mdist[p]), ptr(midx[p]), ptr(mtn[p]), ptr(mcnt[p:])) for p in range(P)]
    for name, radius, flags in modes:
        def many(radius=radius, flags=flags):
            check(lib.affnet_match_ratio_many(ctx, ptr(A), P * T, ptr(B), P * T, 128, ptr(LB), ptr(table), P, T, T, radius, 0.8, INF, flags, 0, ptr(mdist), ptr(midx),
                                              ptr(mtn), ptr(mcnt), ptr(mscratch), st), ctx, "affnet_match_ratio_many")

        def loop(radius=radius, flags=flags):
            for a, b, lb, d, i, t, c in seg:
                check(lib.affnet_match_ratio(ctx, a, T, b, T, 128, lb, radius, 0.8, INF, flags, 0, d, i, t, c, ptr(sscratch), st), ctx, "affnet_match_ratio")
        variants["many_%s_P%d_T%d" % (name, P, T)] = (many, mcnt, keep, max(args.calls // 10, 1))
        variants["loop_%s_P%d_T%d" % (name, P, T)] = (loop, mcnt, keep, max(args.calls // 10, 1))
    kept = {}
    for name, (fn, cnt, _, _) in variants.items():        # warm-up of every shape, and what each call keeps
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        kept[name] = int(cnt.sum().item())
    ms = {name: [] for name in variants}
    for _ in range(args.windows):                        # alternate the variants window by window
        for name, (fn, _, _, calls) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / calls)
    res = {"tool": "ratio_match_rate", "calls_per_window": args.calls, "windows": args.windows, "device": torch.cuda.get_device_name(0),
           "chunks": chunks,
           "ms_per_call": {n: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in ms.items()},
           "kept": kept}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
