#!/usr/bin/env python3
"""Inverted file over int8 rows against the float inverted file: affnet_ivf_search_q8 and affnet_ivf_search (csrc/ivf.hip) for n1 query
descriptors against an index of n2 rows in n_cells = the power of two nearest sqrt(n2) k-means cells - the same codebook for both - in the same
process on the same library build.  HIP events around each call, 3 warm-ups, median of 20 with min - max (tools/ivf_rate.py's timer, database
and queries).

    python tools/ivf_q8_rate.py [--n1 2000] [--n2 65536 1048576] [--k 1 2 8] [--nprobe 1 2 4 8] [--iters 10] [--out FILE]

The time is the whole call: coarse step, grouping, tiles, merge; the quantisation of the query rows (affnet_quantize_desc, what ivf_knn_q8 runs
in front of the int8 call) is timed on its own.  Recall = the share of query rows whose slot 0 is the exhaustive search's: the int8 inverted file
against affnet_knn_q8 (the same distances: what is missed lies outside the probed cells) and against affnet_knn, the float inverted file against
affnet_knn.  With every cell probed the first must be 1.0; that is checked once per n2 on a codebook of 8 cells.  One JSON line per
(n2, input, k); the device bytes of both index kinds are read from the tensors' sizes."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ivf_rate import timed, unit  # noqa: E402


def nbytes(*tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors))


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
        cent = R.train_cells(db, n_cells, iters=args.iters)
        scale = R.quantization_scale(db)
        dbq, dbsq = R.quantize(db, scale)
        pf, p8 = R.IVFParts(db, cent), R.IVFQ8Parts(db, cent, scale, dbq, dbsq)
        assert torch.equal(pf.perm, p8.perm) and torch.equal(pf.cell_start, p8.cell_start), "one codebook, one layout"
        sizes = (p8.cell_start[1:] - p8.cell_start[:-1]).cpu()
        build = {"n_cells": n_cells, "train_iters": args.iters, "scale": round(scale, 4), "cell_rows_min": int(sizes.min()),
                 "cell_rows_median": int(sizes.median()), "cell_rows_max": int(sizes.max()), "empty_cells": int((sizes == 0).sum()),
                 # what an index of each kind holds on the device for its rows (the image tables and the centroids are the same for both)
                 "ivf_index_bytes": nbytes(db, pf.sorted, pf.sorted_sq, pf.perm), "ivf_q8_index_bytes": nbytes(p8.sorted_q, p8.sorted_sq, p8.perm),
                 "ivf_q8_keep_float_bytes": nbytes(db, dbq, dbsq, p8.sorted_q, p8.sorted_sq, p8.perm), "centroid_bytes": nbytes(cent)}
        # every cell probed: the lists are affnet_knn_q8's for every row
        small = R.IVFQ8Parts(db, R.train_cells(db, 8, iters=2), scale, dbq, dbsq)
        for name, q in queries.items():
            qq, qsq = R.quantize(q, scale)
            want = R.knn_q8(qq, qsq, dbq, dbsq, 2, scale)
            got = R.ivf_knn_q8(q, small, 2, 8)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), "all cells probed: not affnet_knn_q8's lists"
        build["all_cells_probed_recall"] = 1.0
        del small
        for name, q in queries.items():
            qq, qsq = R.quantize(q, scale)
            for k in args.k:
                dist = torch.empty(n1, k, dtype=torch.float32, device=dev)
                idx = torch.empty(n1, k, dtype=torch.int32, device=dev)
                dist2 = torch.empty(n1, k, dtype=torch.int32, device=dev)
                s_knn = torch.empty(lib.affnet_knn_scratch_bytes(n1, n2, k, 0), dtype=torch.uint8, device=dev)
                s_q8 = torch.empty(lib.affnet_knn_q8_scratch_bytes(n1, n2, k, lib.affnet_knn_q8_chunks(ctx, n1, n2)), dtype=torch.uint8, device=dev)
                s_ivf = torch.empty(lib.affnet_ivf_scratch_bytes(n1, n_cells, max(args.nprobe), k), dtype=torch.uint8, device=dev)
                s_ivf8 = torch.empty(lib.affnet_ivf_q8_scratch_bytes(n1, n_cells, max(args.nprobe), k), dtype=torch.uint8, device=dev)

                def quant():
                    check(lib.affnet_quantize_desc(ctx, ptr(q), n1, 128, scale, ptr(qq), ptr(qsq), st), ctx, "affnet_quantize_desc")

                def ivf(nprobe):
                    check(lib.affnet_ivf_search(ctx, ptr(q), n1, ptr(pf.sorted), ptr(pf.sorted_sq), ptr(pf.perm), n2, ptr(pf.cell_start), ptr(pf.centroids),
                                                n_cells, 128, k, nprobe, 0, 0, ptr(dist), ptr(idx), None, ptr(s_ivf), st), ctx, "affnet_ivf_search")

                def ivf8(nprobe):
                    check(lib.affnet_ivf_search_q8(ctx, ptr(q), ptr(qq), ptr(qsq), n1, ptr(p8.sorted_q), ptr(p8.sorted_sq), ptr(p8.perm), n2,
                                                   ptr(p8.cell_start), ptr(p8.centroids), n_cells, 128, k, nprobe, 0, 0, scale, ptr(dist2), ptr(dist), ptr(idx),
                                                   None, ptr(s_ivf8), st), ctx, "affnet_ivf_search_q8")
                row = {"tool": "ivf_q8_rate", "n1": n1, "n2": n2, "input": name, "k": k}
                row.update(build)
                check(lib.affnet_knn_q8(ctx, ptr(qq), ptr(qsq), n1, ptr(dbq), ptr(dbsq), n2, 128, k, 0, 0, 0, scale, ptr(dist2), ptr(dist), ptr(idx), ptr(s_q8),
                                        st), ctx, "affnet_knn_q8")
                q8_first, q8_first_d2 = idx[:, 0].clone(), dist2[:, 0].clone()
                check(lib.affnet_knn(ctx, ptr(q), n1, ptr(db), n2, 128, k, 0, 0, 0, ptr(dist), ptr(idx), ptr(s_knn), st), ctx, "affnet_knn")
                first = idx[:, 0].clone()
                row["knn_q8_recall"] = round(float((q8_first == first).float().mean()), 4)
                row["quantize_ms"] = timed(quant)
                for key in ("ivf_ms", "ivf_q8_ms", "ivf_q8_over_ivf", "ivf_recall", "ivf_q8_recall", "ivf_q8_recall_vs_knn_q8"):
                    row[key] = {}
                for nprobe in args.nprobe:
                    s = str(nprobe)
                    row["ivf_ms"][s] = timed(lambda: ivf(nprobe))
                    row["ivf_recall"][s] = round(float((idx[:, 0] == first).float().mean()), 4)
                    row["ivf_q8_ms"][s] = timed(lambda: ivf8(nprobe))
                    hit = idx[:, 0] == q8_first
                    assert dist2[:, 0][hit].equal(q8_first_d2[hit]), "a common neighbour at another distance"
                    row["ivf_q8_recall_vs_knn_q8"][s] = round(float(hit.float().mean()), 4)
                    row["ivf_q8_recall"][s] = round(float((idx[:, 0] == first).float().mean()), 4)
                    row["ivf_q8_over_ivf"][s] = round(row["ivf_q8_ms"][s][0] / row["ivf_ms"][s][0], 4)
                row["device"] = torch.cuda.get_device_name(0)
                print(json.dumps(row), flush=True)
                lines.append(json.dumps(row))
        del db, dbq, dbsq, pf, p8
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
