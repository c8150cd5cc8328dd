#!/usr/bin/env python3
"""Time of one epipolar verification (affnet_epipolar_verify: prep + solve + score + select + refit) at T = 500 and T = 2000 tentatives with
rounds = 8 and 32, next to affnet_verify_matches (homography) at the same T, in the same process on the same library build.

    python tools/epipolar_rate.py [--calls 50] [--windows 7] [--out FILE]

Each figure is the time between two device events around `--calls` back-to-back calls on caller-owned buffers (no allocation, no read-back in the
window), divided by the number of calls; every variant is warmed up first, the windows of all variants alternate, and median / min / max over the
windows are reported, so the spread is visible next to the number.  Input: a planted two-view scene with depth (half the rows replaced by random
frames), generated from a seed.  Fails without a GPU.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = np.array([[800.0, 0.0, 500.0], [0.0, 800.0, 375.0], [0.0, 0.0, 1.0]])
ROT = np.array([[np.cos(0.25), 0.0, np.sin(0.25)], [0.0, 1.0, 0.0], [-np.sin(0.25), 0.0, np.cos(0.25)]])
TRANS = np.array([-1.5, 0.1, 0.3])


def random_frames(rng, n):
    c = np.stack([rng.uniform(50, 950, n), rng.uniform(50, 700, n)], 1)
    s, k = rng.uniform(8, 40, n), rng.uniform(1, 2, n)
    a, b = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    rot = lambda t: np.stack([np.stack([np.cos(t), -np.sin(t)], 1), np.stack([np.sin(t), np.cos(t)], 1)], 1)
    D = np.zeros((n, 2, 2))
    D[:, 0, 0], D[:, 1, 1] = np.sqrt(k), 1.0 / np.sqrt(k)
    return np.concatenate([s[:, None, None] * (rot(a) @ D @ rot(b)), c[:, :, None]], 2)


def scene(T, seed):
    """Every point at its own depth on its own tilted plane; frame 2 = frame 1 through the local linearisation of that plane's homography."""
    rng = np.random.default_rng(seed)
    l1 = random_frames(rng, T)
    depth, tilt, phi = rng.uniform(4, 10, T), rng.uniform(0, 0.8, T), rng.uniform(0, 2 * np.pi, T)
    Ki = np.linalg.inv(K)
    l2 = np.empty_like(l1)
    for i in range(T):
        x = np.array([l1[i, 0, 2], l1[i, 1, 2], 1.0])
        n = np.array([np.sin(tilt[i]) * np.cos(phi[i]), np.sin(tilt[i]) * np.sin(phi[i]), np.cos(tilt[i])])
        H = K @ (ROT + np.outer(TRANS, n) / (n @ (depth[i] * (Ki @ x)))) @ Ki
        p = H @ x
        J = (H[:2, :2] - np.outer(p[:2] / p[2], H[2, :2])) / p[2]
        l2[i, :, :2], l2[i, :, 2] = J @ l1[i, :, :2], p[:2] / p[2]
    l2[:, :, 2] += rng.normal(0.0, 0.3, (T, 2))
    out = rng.uniform(0, 1, T) < 0.5
    l2[out] = random_frames(rng, T)[out]
    perm = rng.permutation(T)
    l2s = np.empty_like(l2)
    l2s[perm] = l2
    return l1.astype(np.float32), l2s.astype(np.float32), np.stack([np.arange(T), perm], 1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("epipolar_rate: no GPU - a time is measured on the device or not at all")
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device("cuda:0")
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    variants = {}
    for T in (500, 2000):
        l1, l2, tent = (torch.from_numpy(a).to(dev) for a in scene(T, T))
        F = torch.zeros(9, dtype=torch.float64, device=dev)
        inl = torch.zeros(T, dtype=torch.uint8, device=dev)
        summ = torch.zeros(4, dtype=torch.int32, device=dev)
        keep = [l1, l2, tent, F, inl, summ]
        for rounds in (8, 32):
            counts = torch.zeros(T * rounds, dtype=torch.int32, device=dev)
            scratch = torch.empty(lib.affnet_epipolar_scratch_bytes(T, rounds), dtype=torch.uint8, device=dev)

            def epi(l1=l1, l2=l2, tent=tent, T=T, rounds=rounds, counts=counts, scratch=scratch, F=F, inl=inl, summ=summ):
                check(lib.affnet_epipolar_verify(ctx, ptr(l1), T, ptr(l2), T, ptr(tent), None, T, 2.0, rounds, 0, 3, ptr(counts), ptr(F), ptr(inl), ptr(summ),
                                                 ptr(scratch), st), ctx, "affnet_epipolar_verify")
            variants["epipolar_T%d_r%d" % (T, rounds)] = (epi, summ, keep + [counts, scratch])
        counts_h = torch.zeros(T, dtype=torch.int32, device=dev)
        scratch_h = torch.empty(lib.affnet_verify_scratch_bytes(T), dtype=torch.uint8, device=dev)
        summ_h = torch.zeros(4, dtype=torch.int32, device=dev)

        def hom(l1=l1, l2=l2, tent=tent, T=T, counts=counts_h, scratch=scratch_h, F=F, inl=inl, summ=summ_h):
            check(lib.affnet_verify_matches(ctx, ptr(l1), T, ptr(l2), T, ptr(tent), None, T, 3.0, 1, 3, ptr(counts), ptr(F), ptr(inl), ptr(summ), ptr(scratch), st),
                  ctx, "affnet_verify_matches")
        variants["homography_T%d" % T] = (hom, summ_h, keep + [counts_h, scratch_h])
    summaries = {}
    for name, (fn, summ, _) in variants.items():        # warm-up of every shape, and what each call finds
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        summaries[name] = summ.cpu().tolist()
    ms = {name: [] for name in variants}
    for _ in range(args.windows):                        # alternate the variants window by window
        for name, (fn, _, _) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / args.calls)
    res = {"tool": "epipolar_rate", "calls_per_window": args.calls, "windows": args.windows, "device": torch.cuda.get_device_name(0),
           "ms_per_call": {n: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in ms.items()},
           "summary": summaries}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
