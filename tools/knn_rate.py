#!/usr/bin/env python3
"""Descriptor index rate: affnet_knn (csrc/knn.hip) for n1 query descriptors against a database of n2, in the same process on the same library
build.  HIP events around each variant, 3 warm-ups, median of 20.

    python tools/knn_rate.py [--n1 2000] [--n2 2000 65536 1048576] [--k 1 2 8] [--out FILE]

Per (n2, k) it times
  * affnet_knn with n_chunks = 1 (every workgroup walks the whole database, the matcher's shape),
  * affnet_knn with the library's own choice (affnet_knn_chunks), and a sweep of n_chunks around it - the floor of tiles per chunk in
    affnet_knn_chunks is set from this sweep,
  * what the library offered before: affnet_distance_matrix followed by torch.topk(k, largest=False); its n1 x n2 matrix is 8 GB at the largest
    size, and the row is skipped with a printed reason if the allocation fails,
and at k = 1, n2 = 2000 also affnet_match_snn, for scale.  Unit random descriptors.  One JSON line per (n2, k); `mfma_fraction` is the rate of the
library's choice on 2 n1 n2 128 FLOP against the 157.3 TFLOP/s fp32 matrix peak."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_MFMA = 157.3e12


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
    ap.add_argument("--n2", type=int, nargs="+", default=[2000, 65536, 1048576])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from affnet_amd import engine
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device("cuda:0")
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    n1 = args.n1
    q = unit(n1, 1, dev)
    lines = []
    for n2 in args.n2:
        db = unit(n2, 2, dev)
        tiles = (n2 + 15) // 16
        auto = lib.affnet_knn_chunks(ctx, n1, n2)
        sweep = sorted(set([c for c in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256) if c <= tiles] + [auto]))
        for k in args.k:
            dist = torch.empty(n1, k, dtype=torch.float32, device=dev)
            idx = torch.empty(n1, k, dtype=torch.int32, device=dev)
            scratch = torch.empty(lib.affnet_knn_scratch_bytes(n1, n2, k, max(sweep)), dtype=torch.uint8, device=dev)

            def knn(nc):
                check(lib.affnet_knn(ctx, ptr(q), n1, ptr(db), n2, 128, k, 0, 0, nc, ptr(dist), ptr(idx), ptr(scratch), st), ctx, "affnet_knn")
            knn(1)
            ref = (dist.clone(), idx.clone())
            row = {"tool": "knn_rate", "n1": n1, "n2": n2, "k": k, "auto_chunks": auto, "tiles_per_chunk": -(-tiles // auto), "sweep_ms": {}}
            for nc in sweep:
                knn(nc)
                assert torch.equal(idx, ref[1]) and dist.view(torch.int32).equal(ref[0].view(torch.int32)), "the result depends on n_chunks = %d" % nc
                med, lo, hi = timed(lambda: knn(nc))
                row["sweep_ms"][str(nc)] = round(med, 4)
                if nc == 1:
                    row["one_chunk_ms"], row["one_chunk_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
            med, lo, hi = timed(lambda: knn(0))
            row["auto_ms"], row["auto_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
            row["mfma_fraction"] = round(2.0 * n1 * n2 * 128 / (med * 1e-3) / PEAK_FP32_MFMA, 4)
            # the path without the index: the full matrix in HBM, then torch.topk
            try:
                full = torch.empty(n1, n2, dtype=torch.float32, device=dev)
                ms = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=dev)

                def matrix_topk():
                    check(lib.affnet_distance_matrix(ctx, ptr(q), n1, ptr(db), n2, 128, ptr(full), ptr(ms), st), ctx, "affnet_distance_matrix")
                    return torch.topk(full, k, dim=1, largest=False)
                med, lo, hi = timed(matrix_topk)
                row["matrix_topk_ms"], row["matrix_topk_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
                del full, ms
            except (RuntimeError, MemoryError) as e:          # torch.OutOfMemoryError is a RuntimeError
                row["matrix_topk_ms"] = None
                print("n2 = %d, k = %d: distance matrix + topk skipped (%d x %d floats = %.1f GB): %s" % (n2, k, n1, n2, 4e-9 * n1 * n2, str(e).splitlines()[0]),
                      flush=True)
                torch.cuda.empty_cache()
            if k == 1 and n2 == 2000:
                md, md2 = torch.empty(n1, device=dev), torch.empty(n1, device=dev)
                mi, tent, cnt = torch.empty(n1, dtype=torch.int32, device=dev), torch.empty(n1, 2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
                ms = torch.empty(lib.affnet_match_scratch_bytes(n1, n2), dtype=torch.uint8, device=dev)

                def snn():
                    check(lib.affnet_match_snn(ctx, ptr(q), n1, ptr(db), n2, 128, 0.8, ptr(md), ptr(mi), ptr(md2), ptr(tent), ptr(cnt), ptr(ms), st), ctx, "affnet_match_snn")
                row["match_snn_ms"] = round(timed(snn)[0], 4)
            row["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(row), flush=True)
            lines.append(json.dumps(row))
        del db
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
