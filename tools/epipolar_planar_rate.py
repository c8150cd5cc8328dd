#!/usr/bin/env python3
"""Time of one plane-aware epipolar verification (affnet_epipolar_verify_planar) at T = 2000 tentatives, rounds = 8, next to the two calls
it contains - affnet_verify_matches (homography, plane_th) and affnet_epipolar_verify - in the same process on the same library build.

    python tools/epipolar_planar_rate.py [--calls 50] [--windows 7] [--out FILE]

Measured as tools/epipolar_rate.py measures: device events around `--calls` back-to-back calls on caller-owned buffers, every variant warmed
up, the windows of all variants alternating, median / min / max over the windows.  Input: a wall with things in front of it - 1200 matches
on one plane, 160 at their own depths, 640 random - generated from a seed.  Fails without a GPU.  Prints one JSON line (and writes it to
--out); "contained_sum" is the sum of the two contained calls' medians, "extra" what the new stages add to it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from epipolar_rate import K, ROT, TRANS, random_frames  # noqa: E402

PLANE_N, PLANE_D = np.array([np.sin(0.3), 0.0, np.cos(0.3)]), 6.0


def scene(T, n_plane, n_off, seed):
    rng = np.random.default_rng(seed)
    l1 = random_frames(rng, T)
    depth, tilt, phi = rng.uniform(3, 10, T), rng.uniform(0, 0.8, T), rng.uniform(0, 2 * np.pi, T)
    role = np.full(T, 2)
    order = rng.permutation(T)
    role[order[:n_plane]], role[order[n_plane:n_plane + n_off]] = 0, 1
    Ki = np.linalg.inv(K)
    l2 = np.empty_like(l1)
    for i in range(T):
        x = np.array([l1[i, 0, 2], l1[i, 1, 2], 1.0])
        n = np.array([np.sin(tilt[i]) * np.cos(phi[i]), np.sin(tilt[i]) * np.sin(phi[i]), np.cos(tilt[i])])
        H = K @ (ROT + (np.outer(TRANS, PLANE_N) / PLANE_D if role[i] == 0 else np.outer(TRANS, n) / (n @ (depth[i] * (Ki @ x))))) @ Ki
        p = H @ x
        J = (H[:2, :2] - np.outer(p[:2] / p[2], H[2, :2])) / p[2]
        l2[i, :, :2], l2[i, :, 2] = J @ l1[i, :, :2], p[:2] / p[2]
    l2[:, :, 2] += rng.normal(0.0, 0.3, (T, 2))
    l2[role == 2] = random_frames(rng, T)[role == 2]
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
        sys.exit("epipolar_planar_rate: no GPU - a time is measured on the device or not at all")
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device("cuda:0")
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    T, rounds = 2000, 8
    l1, l2, tent = (torch.from_numpy(a).to(dev) for a in scene(T, 1200, 160, 7))
    F, H = (torch.zeros(9, dtype=torch.float64, device=dev) for _ in range(2))
    inl, pinl = (torch.zeros(T, dtype=torch.uint8, device=dev) for _ in range(2))
    ints = torch.zeros(5, 4, dtype=torch.int32, device=dev)        # planar: summary, plane summary, info; the two contained calls' summaries
    counts, counts_e = (torch.zeros(T * rounds, dtype=torch.int32, device=dev) for _ in range(2))
    counts_h = torch.zeros(T, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.affnet_epipolar_planar_scratch_bytes(T, rounds), dtype=torch.uint8, device=dev)
    scratch_e = torch.empty(lib.affnet_epipolar_scratch_bytes(T, rounds), dtype=torch.uint8, device=dev)
    scratch_h = torch.empty(lib.affnet_verify_scratch_bytes(T), dtype=torch.uint8, device=dev)

    def planar():
        check(lib.affnet_epipolar_verify_planar(ctx, ptr(l1), T, ptr(l2), T, ptr(tent), None, T, 2.0, 3.0, rounds, 0, 3, ptr(counts), ptr(F), ptr(inl), ptr(ints[0]),
                                                ptr(H), ptr(pinl), ptr(ints[1]), ptr(ints[2]), ptr(scratch), st), ctx, "affnet_epipolar_verify_planar")

    def epi():
        check(lib.affnet_epipolar_verify(ctx, ptr(l1), T, ptr(l2), T, ptr(tent), None, T, 2.0, rounds, 0, 3, ptr(counts_e), ptr(F), ptr(inl), ptr(ints[3]),
                                         ptr(scratch_e), st), ctx, "affnet_epipolar_verify")

    def hom():
        check(lib.affnet_verify_matches(ctx, ptr(l1), T, ptr(l2), T, ptr(tent), None, T, 3.0, 1, 3, ptr(counts_h), ptr(H), ptr(pinl), ptr(ints[4]), ptr(scratch_h), st),
              ctx, "affnet_verify_matches")
    variants = {"planar_T2000_r8": planar, "epipolar_T2000_r8": epi, "homography_T2000": hom}
    summaries = {}
    for name, fn in variants.items():        # warm-up of every variant, and what each call finds
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        summaries[name] = ints.cpu().tolist()[:3] if fn is planar else ints.cpu().tolist()[3 if fn is epi else 4]
    ms = {name: [] for name in variants}
    for _ in range(args.windows):            # alternate the variants window by window
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / args.calls)
    med = {n: statistics.median(v) for n, v in ms.items()}
    both = med["epipolar_T2000_r8"] + med["homography_T2000"]
    res = {"tool": "epipolar_planar_rate", "calls_per_window": args.calls, "windows": args.windows, "device": torch.cuda.get_device_name(0),
           "ms_per_call": {n: {"median": round(med[n], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in ms.items()},
           "contained_sum": round(both, 4), "extra": round(med["planar_T2000_r8"] - both, 4), "summary": summaries}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
