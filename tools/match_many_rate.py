#!/usr/bin/env python3
"""Shortlist re-ranking rate: P image pairs matched and spatially verified as a loop of match_and_verify (one pair per call, the baseline)
against one match_and_verify_many, in the same process on the same library build.  HIP events around each variant, 3 warm-ups, median of 20.

    python tools/match_many_rate.py [--pairs 32] [--n 2000] [--shared-query]

Synthetic input: per pair, image 1 has n random affine frames and unit descriptors; half of image 2's rows are those frames through one homography
with a noisy copy of the descriptor (at shuffled positions), the other half independent.  --shared-query: one image 1 for all pairs (a query against
a shortlist) instead of P different ones.  Prints one JSON line; `readbacks` are the host read-backs (Tensor.cpu / .item / .tolist on a device tensor)
counted in one extra, untimed run of each variant."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H_PLANTED = [[0.88, 0.31, -40.0], [-0.18, 0.94, 150.0], [2e-4, -1e-5, 1.0]]


def random_frames(g, n):
    c = torch.rand(n, 2, generator=g) * torch.tensor([900.0, 650.0]) + 50.0
    s = 8.0 + 32.0 * torch.rand(n, generator=g)
    an = 1.0 + torch.rand(n, generator=g)
    t1, t2 = 2 * math.pi * torch.rand(n, generator=g), 2 * math.pi * torch.rand(n, generator=g)
    rot = lambda t: torch.stack([torch.cos(t), -torch.sin(t), torch.sin(t), torch.cos(t)], 1).view(n, 2, 2)
    D = torch.zeros(n, 2, 2)
    D[:, 0, 0], D[:, 1, 1] = s * an.sqrt(), s / an.sqrt()
    return torch.cat([rot(t1) @ D @ rot(t2), c.view(n, 2, 1)], 2).contiguous()


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def image1(n, seed):
    g = torch.Generator().manual_seed(seed)
    return unit(torch.randn(n, 128, generator=g)), random_frames(g, n)


def image2(d1, l1, seed, dev):
    """The partner of (d1, l1): rows [0, n/2) planted, the rest independent, then shuffled."""
    from affnet_amd import ReprojectionStuff as RS
    n = d1.size(0)
    g = torch.Generator().manual_seed(seed)
    l2 = RS.reprojectLAFs(l1.to(dev), torch.tensor(H_PLANTED)).cpu()
    d2 = d1 + 0.02 * torch.randn(n, 128, generator=g)
    out = torch.arange(n) >= n // 2
    l2[out] = random_frames(g, int(out.sum()))
    d2[out] = torch.randn(int(out.sum()), 128, generator=g)
    perm = torch.randperm(n, generator=g)
    return unit(d2)[perm].contiguous(), l2[perm].contiguous()


def timed(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def count_readbacks(fn):
    n = [0]
    saved = {k: getattr(torch.Tensor, k) for k in ("cpu", "item", "tolist")}

    def wrap(f):
        def g(self, *a, **kw):
            if self.is_cuda:
                n[0] += 1
            return f(self, *a, **kw)
        return g
    try:
        for k, f in saved.items():
            setattr(torch.Tensor, k, wrap(f))
        fn()
    finally:
        for k, f in saved.items():
            setattr(torch.Tensor, k, f)
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--shared-query", action="store_true")
    args = ap.parse_args()
    from affnet_amd import ReprojectionStuff as RS
    dev = torch.device("cuda:0")
    descs, lafs, pairs = [], [], []
    for p in range(args.pairs):
        if p == 0 or not args.shared_query:
            d1, l1 = image1(args.n, 100 + p)
            q = len(descs)
            descs.append(d1.to(dev)); lafs.append(l1.to(dev))
        d2, l2 = image2(d1, l1, 500 + p, dev)
        pairs.append((q, len(descs)))
        descs.append(d2.to(dev)); lafs.append(l2.to(dev))

    def loop():
        return [RS.match_and_verify(descs[a], descs[b], lafs[a], lafs[b]) for a, b in pairs]

    def many():
        return RS.match_and_verify_many(descs, lafs, pairs)

    # the same answers first (the tests assert this; here it guards the comparison)
    for w, g in zip(loop(), many()):
        assert torch.equal(w[0], g[0]) and torch.equal(w[1], g[1]) and torch.equal(w[2], g[2]) and torch.equal(w[3], g[3]) and w[4]["num_inliers"] == g[4]["num_inliers"]
    inl = [r[4]["num_inliers"] for r in many()]
    loop_ms, loop_min = timed(loop)
    many_ms, many_min = timed(many)
    print(json.dumps({"tool": "match_many_rate", "pairs": args.pairs, "n": args.n, "shared_query": bool(args.shared_query), "loop_ms": round(loop_ms, 3),
                      "many_ms": round(many_ms, 3), "loop_over_many": round(loop_ms / many_ms, 3), "loop_min_ms": round(loop_min, 3), "many_min_ms": round(many_min, 3),
                      "readbacks_loop": count_readbacks(loop), "readbacks_many": count_readbacks(many), "median_inliers": int(np.median(inl)),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
