#!/usr/bin/env python3
"""Shortlist re-ranking rate under the epipolar model and with guided matching: P image pairs as a loop of the single-pair call (one pair per call,
the baseline) against the one *_many call, in the same process on the same library build, for three chains:

    fundamental          match_and_verify(model="fundamental")        against match_and_verify_many(model="fundamental")
    guided_homography    match_verify_guided(model="homography")      against match_verify_guided_many(model="homography")
    guided_fundamental   match_verify_guided(model="fundamental")     against match_verify_guided_many(model="fundamental")

HIP events around each variant, 3 warm-ups, median of 20 (with the range).

    python tools/verify_many_rate.py [--pairs 32] [--n 2000] [--shared-query]

The synthetic pairs are tools/match_many_rate.py's (half of image 2 is image 1 through one homography, so under the fundamental model the pairs
are planar scenes: F serves as an inlier test).  Prints one JSON line; `readbacks` are the host read-backs (Tensor.cpu / .item / .tolist on a device
tensor) counted in one extra, untimed run of each variant."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from match_many_rate import count_readbacks, image1, image2  # noqa: E402


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
    return statistics.median(ms), min(ms), max(ms)


def same(w, g):
    """The tuples of a single-pair call and of pair p of the *_many call: the same tensors and the same summary."""
    keys = [k for k in w[4] if k != "counts"]
    return (all(torch.equal(w[i], g[i]) for i in range(4)) and torch.equal(w[4]["counts"], g[4]["counts"]) and
            {k: w[4][k] for k in keys} == {k: g[4][k] for k in keys} and set(w[4]) == set(g[4]))


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

    chains = {
        "fundamental": (lambda: [RS.match_and_verify(descs[a], descs[b], lafs[a], lafs[b], model="fundamental") for a, b in pairs],
                        lambda: RS.match_and_verify_many(descs, lafs, pairs, model="fundamental")),
        "guided_homography": (lambda: [RS.match_verify_guided(descs[a], descs[b], lafs[a], lafs[b], model="homography") for a, b in pairs],
                              lambda: RS.match_verify_guided_many(descs, lafs, pairs, model="homography")),
        "guided_fundamental": (lambda: [RS.match_verify_guided(descs[a], descs[b], lafs[a], lafs[b], model="fundamental") for a, b in pairs],
                               lambda: RS.match_verify_guided_many(descs, lafs, pairs, model="fundamental")),
    }
    out = {}
    for name, (loop, many) in chains.items():
        # the same answers first (the tests assert this; here it guards the comparison)
        res = many()
        for w, g in zip(loop(), res):
            assert same(w, g), name
        loop_ms, loop_min, loop_max = timed(loop)
        many_ms, many_min, many_max = timed(many)
        out[name] = {"loop_ms": round(loop_ms, 3), "many_ms": round(many_ms, 3), "loop_over_many": round(loop_ms / many_ms, 3),
                     "loop_range_ms": [round(loop_min, 3), round(loop_max, 3)], "many_range_ms": [round(many_min, 3), round(many_max, 3)],
                     "readbacks_loop": count_readbacks(loop), "readbacks_many": count_readbacks(many),
                     "median_inliers": int(np.median([r[4]["num_inliers"] for r in res]))}
    print(json.dumps({"tool": "verify_many_rate", "pairs": args.pairs, "n": args.n, "shared_query": bool(args.shared_query), "chains": out,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
