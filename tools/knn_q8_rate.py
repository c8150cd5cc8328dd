#!/usr/bin/env python3
"""Descriptor index rate, int8 against fp32: affnet_knn_q8 (csrc/knn_q8.hip) and affnet_knn (csrc/knn.hip) for n1 query descriptors against a
database of n2, in the same process on the same library build.  HIP events around each variant, 3 warm-ups, median of 20.

    python tools/knn_q8_rate.py [--n1 2000] [--n2 2000 65536 1048576] [--k 1 2 8] [--out FILE]

Per (n2, k) it times
  * affnet_knn_q8 with the library's own choice of chunks (n_chunks = 0: affnet_knn_q8_chunks for k <= 2, about half of it above, where the row
    blocks are half as large) and a sweep of n_chunks around it,
  * affnet_knn with its own choice (affnet_knn_chunks), on the float descriptors the int8 ones were quantised from,
and once per run the quantisation of the n1 queries (affnet_quantize_desc), which a query pays in front of the int8 search and which is
counted separately.  Unit random descriptors, scale = 127 / max|x|.  One JSON line per (n2, k): `speedup` = fp32_ms / q8_ms (search alone),
`staged_gbs` = the database bytes the int8 search's workgroups stage through LDS per second (row blocks x n2 x 128 B), `agree` = the fraction
of query rows whose int8 nearest neighbour is the fp32 one."""
import argparse
import json
import os
import statistics
import sys

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
    from affnet_amd import engine, retrieval
    from affnet_amd._lib import lib, ptr, check
    dev = torch.device("cuda:0")
    ctx, st = engine.utility_ctx(dev), engine.stream_of(dev)
    n1 = args.n1
    q = unit(n1, 1, dev)
    lines = []
    for n2 in args.n2:
        db = unit(n2, 2, dev)
        scale = retrieval.quantization_scale([q, db])
        qq, qsq = retrieval.quantize(q, scale)
        dbq, dbsq = retrieval.quantize(db, scale)
        q_ms = timed(lambda: check(lib.affnet_quantize_desc(ctx, ptr(q), n1, 128, scale, ptr(qq), ptr(qsq), st), ctx, "affnet_quantize_desc"))
        steps = (n2 + 31) // 32
        auto = lib.affnet_knn_q8_chunks(ctx, n1, n2)
        auto32 = lib.affnet_knn_chunks(ctx, n1, n2)
        sweep = sorted(set([c for c in (1, 4, 16, 32, 64, 96, 128, 192, 256, 512) if c <= steps] + [auto]))
        for k in args.k:
            d2 = torch.empty(n1, k, dtype=torch.int32, device=dev)
            dist = torch.empty(n1, k, dtype=torch.float32, device=dev)
            idx = torch.empty(n1, k, dtype=torch.int32, device=dev)
            dist32 = torch.empty(n1, k, dtype=torch.float32, device=dev)
            idx32 = torch.empty(n1, k, dtype=torch.int32, device=dev)
            scratch = torch.empty(lib.affnet_knn_q8_scratch_bytes(n1, n2, k, max(sweep)), dtype=torch.uint8, device=dev)
            scratch32 = torch.empty(lib.affnet_knn_scratch_bytes(n1, n2, k, 0), dtype=torch.uint8, device=dev)

            def knn_q8(nc):
                check(lib.affnet_knn_q8(ctx, ptr(qq), ptr(qsq), n1, ptr(dbq), ptr(dbsq), n2, 128, k, 0, 0, nc, scale, ptr(d2), ptr(dist), ptr(idx), ptr(scratch), st),
                      ctx, "affnet_knn_q8")

            def knn_f32():
                check(lib.affnet_knn(ctx, ptr(q), n1, ptr(db), n2, 128, k, 0, 0, 0, ptr(dist32), ptr(idx32), ptr(scratch32), st), ctx, "affnet_knn")
            knn_q8(1)
            ref = (d2.clone(), dist.clone(), idx.clone())
            rb = 256 if k <= 2 else 128
            row = {"tool": "knn_q8_rate", "n1": n1, "n2": n2, "k": k, "scale": round(scale, 3), "auto_chunks_most": auto,
                   # what n_chunks = 0 takes: k > 2 runs on row blocks of 128 = the choice for 2 n1 rows in blocks of 256
                   "auto_chunks": auto if k <= 2 else lib.affnet_knn_q8_chunks(ctx, 2 * n1, n2),
                   "fp32_auto_chunks": auto32, "sweep_ms": {}, "quantize_queries_ms": round(q_ms[0], 4)}
            for nc in sweep:
                knn_q8(nc)
                assert torch.equal(d2, ref[0]) and torch.equal(idx, ref[2]) and dist.view(torch.int32).equal(ref[1].view(torch.int32)), \
                    "the result depends on n_chunks = %d" % nc
                row["sweep_ms"][str(nc)] = round(timed(lambda: knn_q8(nc))[0], 4)
            med, lo, hi = timed(lambda: knn_q8(0))
            row["q8_ms"], row["q8_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
            row["staged_gbs"] = round(-(-n1 // rb) * n2 * 128 / (med * 1e-3) / 1e9, 1)
            med32, lo, hi = timed(knn_f32)
            row["fp32_ms"], row["fp32_min_max"] = round(med32, 4), [round(lo, 4), round(hi, 4)]
            row["speedup"] = round(med32 / med, 3)
            row["agree"] = round(float((idx[:, 0] == idx32[:, 0]).float().mean()), 4)
            row["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(row), flush=True)
            lines.append(json.dumps(row))
        del db, dbq, dbsq
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
