#!/usr/bin/env python3
"""Time of one guided matching call (affnet_match_guided: norms + prep + forward tiles + merge [+ backward tiles + merge] + selection) for the
planar kind (radius 10 px) and the epipolar kind (radius 4 px), mutual on and off, at 2000 x 2000 and 500 x 500 descriptors, next to
affnet_match_snn on the same descriptors, in the same process on the same library build.

    python tools/guided_rate.py [--calls 50] [--windows 7] [--out FILE]

Each figure is the time between two device events around `--calls` back-to-back calls on caller-owned buffers (no allocation, no read-back in the
window), divided by the number of calls; every variant is warmed up first, the windows of all variants alternate, and median / min / max over the
windows are reported, so the spread is visible next to the number.  Input: planted scenes generated from a seed (half the rows of image 2 replaced
by random frames with random descriptors; the planted rows carry noisy copies of their partner's descriptor), matched under the planted model.
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

from epipolar_rate import K, ROT, TRANS, random_frames, scene  # noqa: E402

PLANTED_H = np.array([[0.88, 0.31, -40.0], [-0.18, 0.94, 150.0], [2e-4, -1e-5, 1.0]])


def planted_F():
    tx = np.array([[0.0, -TRANS[2], TRANS[1]], [TRANS[2], 0.0, -TRANS[0]], [-TRANS[1], TRANS[0], 0.0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ ROT @ Ki
    return F / np.sqrt((F * F).sum())


def planar_scene(T, seed):
    rng = np.random.default_rng(seed)
    l1 = random_frames(rng, T)
    p = np.concatenate([l1[:, :, 2], np.ones((T, 1))], 1) @ PLANTED_H.T
    l2 = l1.copy()
    l2[:, :, 2] = p[:, :2] / p[:, 2:3] + rng.normal(0.0, 0.3, (T, 2))
    out = rng.uniform(0, 1, T) < 0.5
    l2[out] = random_frames(rng, T)[out]
    perm = rng.permutation(T)
    l2s = np.empty_like(l2)
    l2s[perm] = l2
    return l1.astype(np.float32), l2s.astype(np.float32), np.stack([np.arange(T), perm], 1).astype(np.int32)


def descriptors(tent, seed):
    """Unit rows: image 2 random, image 1 a noisy copy of its partner's row - which is a planted partner only where the frames agree."""
    rng = np.random.default_rng(seed)
    T = len(tent)
    d2 = rng.normal(size=(T, 128))
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    d1 = d2[tent[:, 1]] + 0.03 * rng.normal(size=(T, 128))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    return d1.astype(np.float32), d2.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("guided_rate: no GPU - a time is measured on the device or not at all")
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device("cuda:0")
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    variants = {}
    for T in (500, 2000):
        for kind, name, radius, model, frames in ((0, "planar", 10.0, PLANTED_H, planar_scene), (1, "epipolar", 4.0, planted_F(), scene)):
            l1, l2, tent = frames(T, T)
            d1, d2 = descriptors(tent, T + kind)
            D1, D2, L1, L2 = (torch.from_numpy(a).to(dev) for a in (d1, d2, l1, l2))
            M = torch.from_numpy(np.ascontiguousarray(model, np.float64).reshape(9)).to(dev)
            dist = torch.zeros(T, 2, dtype=torch.float32, device=dev)
            idx = torch.zeros(T, 2, dtype=torch.int32, device=dev)
            tn = torch.zeros(T, 2, dtype=torch.int32, device=dev)
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            scratch = torch.empty(lib.affnet_match_guided_scratch_bytes(T, T, 0), dtype=torch.uint8, device=dev)
            keep = [D1, D2, L1, L2, M, dist, idx, tn, scratch]
            for mutual in (1, 0):
                def guided(D1=D1, D2=D2, L1=L1, L2=L2, M=M, T=T, kind=kind, radius=radius, mutual=mutual, dist=dist, idx=idx, tn=tn, cnt=cnt, scratch=scratch):
                    check(lib.affnet_match_guided(ctx, ptr(D1), T, ptr(D2), T, 128, ptr(L1), ptr(L2), ptr(M), kind, radius, 0.9, float("inf"), mutual, 0, None,
                                                  ptr(dist), ptr(idx), ptr(tn), ptr(cnt), ptr(scratch), st), ctx, "affnet_match_guided")
                variants["guided_%s_%s_T%d" % (name, "mutual" if mutual else "oneway", T)] = (guided, cnt, keep)
            md, md2 = torch.zeros(T, device=dev), torch.zeros(T, device=dev)
            mi = torch.zeros(T, dtype=torch.int32, device=dev)
            tn2 = torch.zeros(T, 2, dtype=torch.int32, device=dev)
            cnt2 = torch.zeros(1, dtype=torch.int32, device=dev)
            scratch2 = torch.empty(lib.affnet_match_scratch_bytes(T, T), dtype=torch.uint8, device=dev)

            def snn(D1=D1, D2=D2, T=T, md=md, mi=mi, md2=md2, tn2=tn2, cnt2=cnt2, scratch2=scratch2):
                check(lib.affnet_match_snn(ctx, ptr(D1), T, ptr(D2), T, 128, 0.8, ptr(md), ptr(mi), ptr(md2), ptr(tn2), ptr(cnt2), ptr(scratch2), st), ctx,
                      "affnet_match_snn")
            variants["match_snn_%s_T%d" % (name, T)] = (snn, cnt2, keep + [md, md2, mi, tn2, scratch2])
    kept = {}
    for name, (fn, cnt, _) in variants.items():        # warm-up of every shape, and what each call keeps
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        kept[name] = int(cnt.item())
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
    res = {"tool": "guided_rate", "calls_per_window": args.calls, "windows": args.windows, "device": torch.cuda.get_device_name(0),
           "tile_skipping": "not built",
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
