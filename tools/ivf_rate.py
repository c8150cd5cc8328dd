#!/usr/bin/env python3
"""Inverted-file search rate and recall: affnet_ivf_search (csrc/ivf.hip) for n1 query descriptors against an index of n2 rows in
n_cells = the power of two nearest sqrt(n2) k-means cells, next to the two exhaustive searches affnet_knn and affnet_knn_q8 on the same rows, in
the same process on the same library build.  HIP events around each variant, 3 warm-ups, median of 20 with min - max.

    python tools/ivf_rate.py [--n1 2000] [--n2 65536 1048576] [--k 1 2 8] [--nprobe 1 2 4 8] [--iters 10] [--out FILE]

The time is the whole affnet_ivf_search call: coarse step, grouping, tiles, merge.  The recall is the share of query rows whose nearest
neighbour (slot 0) is affnet_knn's, on two inputs over the same unit random database:
  * random:  unit random query rows - the worst case, their distances to all database rows concentrate;
  * planted: query row r = database row (r * n2) // n1 with 0.005 * normal added and renormalised (the noisy copies of tests/_knn_fp64.py).
One JSON line per (n2, input, k); the codebook training time (train_cells, all rows) and the cell sizes are reported once per n2."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]


def unit(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(n, 128)
    for r in range(0, n, 1 << 16):          # in pieces: the host generator is slow on one large call
        x = torch.randn(min(1 << 16, n - r), 128, generator=g)
        out[r:r + x.size(0)] = x / x.norm(dim=1, keepdim=True)
    return out.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=2000)
    ap.add_argument("--n2", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from affnet_amd import engine, retrieval as R
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device("cuda:0")
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    n1 = args.n1
    lines = []
    for n2 in args.n2:
        db = unit(n2, 2, dev)
        src = (torch.arange(n1, device=dev) * n2) // n1
        g = torch.Generator().manual_seed(3)
        noisy = db[src] + 0.005 * torch.randn(n1, 128, generator=g).to(dev)
        queries = {"random": unit(n1, 1, dev), "planted": (noisy / noisy.norm(dim=1, keepdim=True)).contiguous()}
        n_cells = R.default_cells(n2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cent = R.train_cells(db, n_cells, iters=args.iters)
        torch.cuda.synchronize()
        train_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        p = R.IVFParts(db, cent)
        torch.cuda.synchronize()
        layout_s = time.perf_counter() - t0
        sizes = (p.cell_start[1:] - p.cell_start[:-1]).cpu()
        build = {"n_cells": n_cells, "train_iters": args.iters, "train_s": round(train_s, 3), "layout_s": round(layout_s, 3),
                 "cell_rows_min": int(sizes.min()), "cell_rows_median": int(sizes.median()), "cell_rows_max": int(sizes.max()),
                 "empty_cells": int((sizes == 0).sum())}
        scale = R.quantization_scale(db)
        dbq, dbsq = R.quantize(db, scale)
        for name, q in queries.items():
            qq, qsq = R.quantize(q, scale)
            for k in args.k:
                dist = torch.empty(n1, k, dtype=torch.float32, device=dev)
                idx = torch.empty(n1, k, dtype=torch.int32, device=dev)
                dist2 = torch.empty(n1, k, dtype=torch.int32, device=dev)
                s_knn = torch.empty(lib.affnet_knn_scratch_bytes(n1, n2, k, 0), dtype=torch.uint8, device=dev)
                s_q8 = torch.empty(lib.affnet_knn_q8_scratch_bytes(n1, n2, k, lib.affnet_knn_q8_chunks(ctx, n1, n2)), dtype=torch.uint8, device=dev)
                s_ivf = torch.empty(lib.affnet_ivf_scratch_bytes(n1, n_cells, max(args.nprobe), k), dtype=torch.uint8, device=dev)

                def knn():
                    check(lib.affnet_knn(ctx, ptr(q), n1, ptr(db), n2, 128, k, 0, 0, 0, ptr(dist), ptr(idx), ptr(s_knn), st), ctx, "affnet_knn")

                def knn_q8():
                    check(lib.affnet_knn_q8(ctx, ptr(qq), ptr(qsq), n1, ptr(dbq), ptr(dbsq), n2, 128, k, 0, 0, 0, scale, ptr(dist2), ptr(dist), ptr(idx),
                                            ptr(s_q8), st), ctx, "affnet_knn_q8")

                def ivf(nprobe):
                    check(lib.affnet_ivf_search(ctx, ptr(q), n1, ptr(p.sorted), ptr(p.sorted_sq), ptr(p.perm), n2, ptr(p.cell_start), ptr(p.centroids),
                                                n_cells, 128, k, nprobe, 0, 0, ptr(dist), ptr(idx), None, ptr(s_ivf), st), ctx, "affnet_ivf_search")
                row = {"tool": "ivf_rate", "n1": n1, "n2": n2, "input": name, "k": k}
                row.update(build)
                row["knn_q8_ms"] = timed(knn_q8)
                q8_first = idx[:, 0].clone()
                row["knn_ms"] = timed(knn)
                first, first_d = idx[:, 0].clone(), dist[:, 0].clone()
                row["knn_q8_recall"] = round(float((q8_first == first).float().mean()), 4)
                row["ivf_ms"], row["ivf_recall"], row["ivf_over_knn"] = {}, {}, {}
                for nprobe in args.nprobe:
                    row["ivf_ms"][str(nprobe)] = timed(lambda: ivf(nprobe))
                    hit = idx[:, 0] == first
                    # a hit reports the exhaustive search's distance, bit for bit
                    assert dist[:, 0][hit].view(torch.int32).equal(first_d[hit].view(torch.int32)), "a common neighbour at another distance"
                    row["ivf_recall"][str(nprobe)] = round(float(hit.float().mean()), 4)
                    row["ivf_over_knn"][str(nprobe)] = round(row["ivf_ms"][str(nprobe)][0] / row["knn_ms"][0], 4)
                if name == "planted":
                    row["knn_finds_source"] = round(float((first.long() == src).float().mean()), 4)
                row["device"] = torch.cuda.get_device_name(0)
                print(json.dumps(row), flush=True)
                lines.append(json.dumps(row))
        del db, dbq, p
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
