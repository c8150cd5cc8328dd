#!/usr/bin/env python
"""Benchmark of the hot path on MI355X (see the contract in DESIGN.md "Measurement").

    python bench.py                                   # N = 1, BASELINE.json configs[2] (the metric's configuration)
    python bench.py --gpus 8                          # self-spawns 8 ranks (one per GPU, RCCL), prints ONE JSON line
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W        # same, launched by torchrun (RANK / LOCAL_RANK / WORLD_SIZE from the env)
    python bench.py --config2                         # BASELINE configs[1]: single-image latency (graf img1, 2000 kp, H2D included)
    python bench.py --config5                         # BASELINE configs[4]: 3840x2160, 8000 kp
    python bench.py --include-h2d                     # headline loop with every step's images uploaded on a copy stream
    python bench.py --full                            # + cpu_baseline, parity_check, the other arithmetic modes, other_configs, secondary_rooflines
    python bench.py --dump-outputs DIR                # + the rows the last timed step returned, as DIR/*.npy (dump_outputs)

A "step" = one pass of the whole hot path (pyramid -> Hessian/NMS detector -> AffNet -> filter ->
OriNet -> level select -> HardNet) over one batch of 64 synthetic 1024x768 images, 2000 keypoints
each (BASELINE.json configs[2], the configuration the metric is quoted on), per rank (weak scaling),
images resident in HBM before the timed region, processed as 2 fused library calls of 32 images (every
kernel launch covers 32 images), followed for N > 1 by the gather of the padded
(count, LAFs, responses, descriptors) records (gather to rank 0, or --gather all = all_gather).  value = keypoints returned by
all ranks / max-over-ranks time.

roofline           : dominant kernel = fused HardNet trunk (cnn32_trunk_kernel<2>, fp32 MFMA).  achieved = algorithmic FLOPs
                     per launch / mean launch duration measured with HIP events around that launch on its own stream inside
                     the timed region (affnet_profile_*).
--full only:
secondary_rooflines: the HBM-bound scale-space / sampler kernels: algorithmic bytes / HIP-event time, fraction of 8 TB/s.
cpu_baseline       : the CPU oracle (port of the reference, same torch CPU operators) on this host's cores on a bounded
                     sample of the same workload (rank 0, N == 1 only): thread-count sweep, then median of 5 images.
parity_check       : the GPU rows of the bench's own batched launches compared with the oracle outputs of the same seeds.
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
T_START = time.time()              # process start (after `import torch`): the JSON line carries the wall time of every section of the run

H, W, NKP, BATCH = 768, 1024, 2000, 64
# algorithmic work: 2*MAC per patch, dense, BN/ReLU/normalisation excluded
FLOP_AFF, FLOP_ORI, FLOP_HARD = 19193856.0, 19316736.0, 78184448.0
FLOP_HARD_HEAD = 2.0 * 8192 * 128
PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, 64 FLOP/clk/SIMD
PEAK_BF16_MFMA_TFLOPS = 16 * 157.3  # MI355X_MICROARCH.md: bf16 MFMA = 16x the fp32 matrix rate (~2.5 PF dense); rooflines of the fp32_split3 lines
PEAK_HBM_GBS = 8000.0              # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec; ~6.3 TB/s achievable)
GRAF = os.path.join(ROOT, "tests", "golden", "graf_img1.png")
DTYPE_SPLIT3 = ("f32 (AFFNET_ARITH_FP32_SPLIT3: every fp32 operand of the CNN contractions as three bf16 terms, six v_mfma_f32_16x16x32_bf16 per "
                "product, fp32 accumulate; conv0, the AffNet / OriNet heads and everything outside the CNNs plain fp32)")
DTYPE_SPLIT2H = ("f32 (AFFNET_ARITH_FP32_SPLIT2H: every fp32 operand of the CNN contractions as two fp16 terms (|x - h - l| <= 2^-23 |x| for |x| >= 2^-2, <= 2^-25 absolute below), three "
                 "v_mfma_f32_16x16x32_f16 per product, fp32 accumulate; conv0, the AffNet / OriNet heads and everything outside the CNNs plain fp32)")
# the split arithmetic modes of the boundary (include/affnet_hip.h): matrix instructions per fp32 product, labels
SPLIT = {"fp32_split3": {"products": 6.0, "dtype": DTYPE_SPLIT3, "label": "CNN contractions on 3 x bf16 split operands", "insn": "6 x v_mfma_f32_16x16x32_bf16"},
         "fp32_split2h": {"products": 3.0, "dtype": DTYPE_SPLIT2H, "label": "CNN contractions on 2 x fp16 split operands", "insn": "3 x v_mfma_f32_16x16x32_f16"}}


# ----------------------------------------------------------------------------------------------------------------------
def pmc_traffic(images_per_launch, split=False):
    # split: False = the exact-fp32 HardNet trunk, "fp32_split3" / "fp32_split2h" (True = fp32_split3) = that mode's instantiation
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE
    in separate passes, tools/gpu_full.sh + tools/pmc_traffic.py; counters cannot be read from inside this process)."""
    import glob
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json"))
                   if "sampler" not in os.path.basename(f) and "config5" not in os.path.basename(f))
    d = k = None
    for f in reversed(files):                  # newest evidence set that has the exact-fp32 HardNet trunk (its name gained template arguments over the rounds)
        d = json.load(open(f))
        names = ("void cnn32_trunk_kernel<2, 8, false, 2>",) if split == "fp32_split2h" else \
                ("void cnn32_trunk_kernel<2, 8, false, 3>", "void cnn32_trunk_kernel<2, 8, false, true>") if split else \
                ("void cnn32_trunk_kernel<2, 8, false, 0>", "void cnn32_trunk_kernel<2, 8, false, false>", "void cnn32_trunk_kernel<2, 8, false>", "void cnn32_trunk_kernel<2, 8>")
        for name in names:
            k = d["kernels"].get(name)
            if k:
                break
        if k:
            files = [f]
            break
    if not k:
        return None, None
    scale = images_per_launch / float(d["images_per_launch"])
    note = "%s: %s; scaled to %d images per launch" % (os.path.basename(files[-1]), d.get("correction", "2 x FETCH_SIZE + WRITE_SIZE"),
                                                     images_per_launch)
    return k["hbm_bytes"] * scale, note


def gpu_state(tag):
    """One rocm-smi sample (clock levels, socket power, power cap) for the JSON line: a run on a box that clocks or caps lower than its
    peers (round 4 saw one box 12 % slower in EVERY stage, both arithmetic modes) can then be told from a regression."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--showmaxpower", "--json"], capture_output=True, text=True, timeout=20,
                             stdin=subprocess.DEVNULL).stdout
        d = json.loads(out[out.index("{"):])
        c = d.get("card0", {})
        keep = {k: v for k, v in c.items() if any(t in k.lower() for t in ("sclk", "mclk", "power"))}
        keep["when"] = tag
        return keep
    except Exception as e:                                   # noqa: BLE001
        return {"when": tag, "error": repr(e)[:200]}


def host_threads():
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or avail
    except Exception:
        phys = avail
    return avail, min(phys, avail)


def cpu_baseline(n_timed=3, n_keep=2, node=True):
    """the oracle harness on this host's cores, same inputs as the GPU run: sweep the intra-op thread
    count on one image (128 SMT threads lose to 8-16 on the GPU box: oversubscribed small convolutions), then 1 warm-up +
    n_timed images at the best setting, median.  Returns (record, oracle outputs of the first n_keep timed images).
    Bounded (a reported baseline, never the target): 3 sweep points, 3 timed images, one node-level configuration
    with one round - ~25 s of the default run."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import affnet_oracle as orc
    sd = {k: torch.load(os.path.join(ROOT, "pretrained", k + ".pth"), map_location="cpu", weights_only=False)["state_dict"]
          for k in ("AffNet", "OriNet")}
    hard = orc.synthetic_hardnet_state(0)

    def one(seed):
        x = orc.synthetic_image(H, W, seed)
        ex = orc.OracleExtractor(mrSize=5.192, num_features=NKP, border=5, num_Baum_iters=1, affnet_sd=sd["AffNet"],
                                 orinet_sd=sd["OriNet"], reproduce_wasted_extraction=True)
        t0 = time.perf_counter()
        L, r, P, D = orc.describe(x, ex, hard, do_ori=True, ps=32)
        return time.perf_counter() - t0, {"keys": ex.keys.numpy().copy(), "LAFs": L.numpy().copy(), "resp": r.numpy().copy(),
                                          "desc": D.numpy().copy(), "ori_norm": ex.ori_vec.norm(dim=1).numpy().copy(),
                                          "ex": ex, "hw": (H, W), "n_out": NKP}      # ex: the run itself, for parity_check's float64 referee

    t_cpu0 = time.time()
    avail, phys = host_threads()
    default_threads = torch.get_num_threads()
    # never more threads than physical cores: measured on the 128-core / 256-thread GPU box, one 1024x768 image takes 1.9 s on 8
    # threads, 3.5 s on 64, 7.2 s on 128 and 298 s (!) on 256 - the small convolutions of this path drown in OpenMP overhead
    cand = sorted({t for t in (8, 16) if 1 <= t <= phys} | ({phys} if phys < 8 else set()))      # 32 threads never won on the 128-core boxes (1.46 - 1.5 s vs 1.5 s at 16)
    one(0)                                              # warm-up (allocator, oneDNN primitive caches)
    sweep = {}
    for t in cand:
        torch.set_num_threads(t)
        sweep[t] = one(0)[0]
        if sweep[t] > 1.2 * min(sweep.values()):        # past the optimum: larger counts only get slower
            break
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    one(0)                                              # warm-up at the chosen setting
    times, kps, kept = [], [], []
    for i in range(1, n_timed + 1):
        dt, out = one(i)
        times.append(dt)
        kps.append(out["LAFs"].shape[0])
        if len(kept) < n_keep:
            kept.append((i, out))
        else:
            out.pop("ex")                               # the extractor holds the image's pyramid
    torch.set_num_threads(default_threads)
    order = sorted(range(n_timed), key=lambda i: times[i])
    med = order[n_timed // 2]
    par = torch.__config__.parallel_info().split("\n")
    rec = {"value": kps[med] / times[med], "unit": "keypoints/s", "cores": best, "kind": "port",
           "threads_used": best, "threads_available": avail, "physical_cores": phys,
           "thread_sweep_s_per_image": {str(k): round(v, 3) for k, v in sweep.items()},
           "seconds_per_image": [round(t, 3) for t in times], "spread": (max(times) - min(times)) / times[med],
           "parallel_info": "; ".join(l.strip() for l in par if "thread" in l.lower() or "OpenMP" in l or "MKL" in l)[:300],
           "sample": "median of %d synthetic %dx%d images x %d kp (seeds 1..%d) after a thread-count sweep on seed 0 and 1 warm-up, "
                     "%.1f s of timed CPU work; oracle/affnet_oracle.py = the reference's torch-CPU operator sequence incl. its "
                     "discarded extra extraction (SparseImgRepresenter.py:178-179)" % (n_timed, W, H, NKP, n_timed, sum(times))}
    rec["seconds_total_single_process"] = round(time.time() - t_cpu0, 1)
    if node:
        t_node0 = time.time()
        try:
            # the whole host: cores/8 processes x 8 threads (the path's small convolutions stop scaling at 8-16 threads; round 3 measured
            # 16 x 8 ahead of 8 x 16 on the 128-core box: 2619 vs 1641 kp/s), one round after a warm-up image per process
            rec["node_throughput"] = cpu_node_throughput(phys, workers=max(1, min(16, phys // 8)), rounds=1)
        except Exception as e:                          # noqa: BLE001  (the single-process figure stands)
            rec["node_throughput"] = {"error": repr(e)[:300]}
        rec["node_throughput"]["seconds_total"] = round(time.time() - t_node0, 1)
    return rec, kept


def cpu_node_throughput(phys, workers=8, rounds=2):
    """The same oracle on the WHOLE host: `workers` processes x (physical cores / workers) threads, one image each per round,
    all started together; keypoints of a round / its wall time, median over the rounds.  One process with every core is not the
    host's best: the path's small convolutions stop scaling at 8-16 threads (thread sweep above)."""
    import subprocess
    workers = max(1, min(workers, phys))
    threads = max(1, phys // workers)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", "%d,%d,%d,%d,%d,%d" % (100 + 10 * i, threads, rounds, H, W, NKP)],
                              stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for i in range(workers)]
    try:
        for p in procs:
            assert p.stdout.readline().strip() == "ready", "cpu worker did not start"
        per_round = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            for p in procs:
                p.stdin.write("go\n"); p.stdin.flush()
            kp = sum(int(p.stdout.readline().strip()) for p in procs)
            per_round.append((kp, time.perf_counter() - t0))
    finally:
        for p in procs:
            try:
                p.stdin.close()
            except Exception:
                pass
            p.wait(timeout=60)
    rates = sorted(k / t for k, t in per_round)
    return {"value": rates[len(rates) // 2], "unit": "keypoints/s", "processes": workers, "threads_per_process": threads, "cores": workers * threads,
            "rounds_s": [round(t, 3) for _, t in per_round],
            "sample": "%d processes x %d threads, one %dx%d image x %d kp each per round, %d round(s) after a small warm-up image (320x240) per process, median" %
                      (workers, threads, W, H, NKP, rounds)}


def cpu_worker(spec):
    """Child of cpu_node_throughput: seed0, threads, rounds, H, W, NKP.  Prints 'ready' after one warm-up image, then for every 'go'
    line on stdin processes one image and prints its keypoint count."""
    global H, W, NKP
    seed0, threads, rounds, H, W, NKP = (int(v) for v in spec.split(","))
    torch.set_num_threads(threads)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import affnet_oracle as orc
    sd = {k: torch.load(os.path.join(ROOT, "pretrained", k + ".pth"), map_location="cpu", weights_only=False)["state_dict"] for k in ("AffNet", "OriNet")}
    hard = orc.synthetic_hardnet_state(0)

    def one(seed):
        ex = orc.OracleExtractor(mrSize=5.192, num_features=NKP, border=5, num_Baum_iters=1, affnet_sd=sd["AffNet"], orinet_sd=sd["OriNet"],
                                 reproduce_wasted_extraction=True)
        L, r, P, D = orc.describe(imgs[seed], ex, hard, do_ori=True, ps=32)
        return int(L.shape[0])

    imgs = {s: orc.synthetic_image(H, W, s) for s in range(seed0 + 1, seed0 + rounds + 1)}     # inputs resident before the timed rounds
    # warm-up on a SMALL image (thread pools, allocator, the oneDNN primitives of the 32 x 32 patch CNNs, which do not depend on the image
    # size): a full-size warm-up image per process cost ~8 s of the run for a figure that is "never the target"
    ex0 = orc.OracleExtractor(mrSize=5.192, num_features=300, border=5, num_Baum_iters=1, affnet_sd=sd["AffNet"], orinet_sd=sd["OriNet"],
                              reproduce_wasted_extraction=True)
    orc.describe(orc.synthetic_image(240, 320, seed0), ex0, hard, do_ori=True, ps=32)
    print("ready", flush=True)
    for k in range(rounds):
        if not sys.stdin.readline():
            break
        print(one(seed0 + 1 + k), flush=True)


GOLDEN_SEEDS = (0, 1, 2, 63)       # tests/golden/synth_768x1024_s{seed}_n2000.npz: the UNMODIFIED reference on the authoring host (tests/golden/make_golden_config3.py)


def golden_check(fetch, batch):
    """Host-independent leg of the parity statement: rows of the bench's own images from the last timed step against the
    committed outputs of the unmodified reference (authoring host) - no live oracle, no referee, the plain BASELINE tolerance.  Rows are matched
    through the bit pattern of the response (the reference emits no integer keys; tests/_rowmatch.py).  Only at the metric's configuration."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _rowmatch import match_rows
    tot = {"seeds": [], "rows": 0, "matched": 0, "rows_outside_1e-3": 0, "laf_max_px": 0.0, "desc_max": 0.0, "desc_rows_outside_1e-3": 0, "same_row_order": True}
    for seed in GOLDEN_SEEDS:
        path = os.path.join(ROOT, "tests", "golden", "synth_%dx%d_s%d_n%d.npz" % (H, W, seed, NKP))
        if seed >= batch or not os.path.isfile(path):
            continue
        g, got = np.load(path), fetch(seed)
        gi, wi = match_rows(got["resp"], got["LAFs"], g["resp"], g["LAFs"])
        dl = np.abs(got["LAFs"][gi] - g["LAFs"][wi]).reshape(len(gi), -1).max(axis=1)
        dd = np.abs(got["desc"][gi] - g["desc"][wi]).max(axis=1)
        tot["seeds"].append(seed)
        tot["rows"] += int(len(g["resp"]))
        tot["matched"] += int(len(gi))
        tot["rows_outside_1e-3"] += int((dl >= 1e-3).sum())
        tot["laf_max_px"] = max(tot["laf_max_px"], float(dl.max()))
        tot["desc_max"] = max(tot["desc_max"], float(dd.max()))
        tot["desc_rows_outside_1e-3"] += int((dd >= 1e-3).sum())
        tot["same_row_order"] &= bool(np.array_equal(gi, wi))
    if not tot["seeds"]:
        return None
    # matched rows carry bit-equal responses by construction of the matching; unmatched = keys only one side returns (borderline shape-filter
    # decisions, accounted for key by key in the live-oracle leg)
    tot["pass"] = bool(tot["matched"] >= 0.995 * tot["rows"] and tot["rows_outside_1e-3"] == 0 and tot["desc_rows_outside_1e-3"] == 0)
    tot["bar"] = ">= 99.5 % of the reference's rows matched by response bit pattern, EVERY matched LAF row within 1e-3 px and every descriptor within 1e-3 (no referee, no budget)"
    tot["reference"] = "tests/golden/synth_%dx%d_s*_n%d.npz: the unmodified reference on the authoring host (tests/golden/make_golden_config3.py)" % (H, W, NKP)
    return tot


def parity_check(kept, fetch, tag=None, golden_batch=0):
    """GPU rows of the benchmark's own batched launches (north_star: LAFs and descriptors within 1e-3), two legs.
    fetch(seed) -> dict(ids, LAFs, resp, desc) numpy arrays of that image from the LAST timed step.
    1. `golden` (golden_check): against the committed outputs of the unmodified reference - host independent, plain tolerance.
    2. Against the oracle run LIVE on this host (its rounding differs per CPU in a few operators: DESIGN section 2), every key and every row
       accounted for (oracle/fp64_referee.py, as in tests/test_gpu_parity.py): a key only one side returns must trace to a borderline decision of
       the reference's shape filter (SparseImgRepresenter.py:147-162) or to the top-N cut it shifted (`unmatched_unexplained` = 0); a matched row
       outside 1e-3 px must be (a) no farther from a float64 evaluation of the post-detector stages than the CPU reference's own row + 1e-3 px, or
       (b) sit on a reference row that is itself >= 1e-3 px from float64, within 4x that error - rows meeting neither are counted
       (`rows_outside_1e-3_beyond_referee`) against the budget stated in fp64_referee.py (1 per 4000 matched rows); no row may be outside 1e-2 px."""
    import numpy as np
    import fp64_referee as rf
    threads_before = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, host_threads()[1])))      # the referee's small float64 GEMMs: more threads only get slower (cpu_baseline's sweep)
    key = lambda a: a[:, 0].astype(np.int64) * (1 << 40) + a[:, 1].astype(np.int64) * (1 << 32) + a[:, 2].astype(np.int64)
    tot = {"images": 0, "seeds": [], "keypoints": 0, "matched": 0, "laf_max_px": 0.0, "laf_rows_within_1e-3": 0, "desc_max": 0.0,
           "desc_rows_within_1e-3": 0, "responses_equal": True, "same_row_order": True, "unmatched_keys": 0, "unmatched_borderline_flips": 0,
           "unmatched_unexplained": 0, "unmatched_rows": [], "rows_worse_than_cpu_vs_fp64": 0, "rows_outside_1e-3_beyond_referee": 0, "beyond_budget": 0, "rows_outside_1e-2": 0,
           "rows_outside_5e-3_unexplained": 0, "rows_outside_1e-3": [], "rows_outside_combined_bar_round4": 0}
    for seed, want in kept:
        got = fetch(seed)
        if os.environ.get("AFFNET_DUMP_ROWS"):          # the HIP path's rows of this seed, for tests/offline_parity_account.py on another host
            os.makedirs(os.environ["AFFNET_DUMP_ROWS"], exist_ok=True)
            np.savez_compressed(os.path.join(os.environ["AFFNET_DUMP_ROWS"], "configs_2__metric_configuration__image_%d__bench_%s.npz" % (seed, tag or "fp32")),
                                ids=got["ids"], LAFs=got["LAFs"], resp=got["resp"], desc=got["desc"])
        kg, kw = key(got["ids"]), key(want["keys"])
        pos = {k: i for i, k in enumerate(kw)}
        gi = np.array([i for i, k in enumerate(kg) if k in pos], dtype=np.int64)
        wi = np.array([pos[kg[i]] for i in gi], dtype=np.int64)
        dl = np.abs(got["LAFs"][gi] - want["LAFs"][wi]).reshape(len(gi), -1).max(axis=1)
        dd = np.abs(got["desc"][gi] - want["desc"][wi]).max(axis=1)
        if "ref" not in want:
            want["ref"] = rf.Referee(want["ex"], want["hw"][1], want["hw"][0])       # cached: the other arithmetic modes ask about the same rows
        acc = rf.parity_account(want["ref"], got["ids"], got["LAFs"], want["n_out"])
        tot["unmatched_keys"] += acc["unmatched_keys"]
        tot["unmatched_borderline_flips"] += acc["unmatched_borderline_flips"]
        tot["unmatched_unexplained"] += acc["unmatched_unexplained"]
        tot["unmatched_rows"] += [dict(r, seed=seed) for r in acc["unmatched_rows"]]
        tot["rows_worse_than_cpu_vs_fp64"] += acc["rows_worse_than_cpu_vs_fp64"]
        tot["rows_outside_1e-3_beyond_referee"] += acc["rows_outside_1e-3_beyond_referee"]
        tot["rows_outside_1e-2"] += acc["rows_outside_1e-2"]
        tot["rows_outside_5e-3_unexplained"] += acc["rows_outside_5e-3_unexplained"]
        # secondary record: round 4's fitted bar max(1e-3 px, S (1e-5 + 4e-5 / |o|)) - not part of `pass`
        Lw = want["LAFs"][wi].astype(np.float64)
        S = np.sqrt(np.abs(Lw[:, 0, 0] * Lw[:, 1, 1] - Lw[:, 0, 1] * Lw[:, 1, 0]))
        on = want["ori_norm"][wi].astype(np.float64) if "ori_norm" in want else None
        bar = np.maximum(1e-3, S * (1e-5 + (0.0 if on is None else 4e-5 / np.maximum(on, 1e-12))))
        tot["rows_outside_combined_bar_round4"] += int((dl > bar).sum())
        ref_rows = {tuple(r["key_octave_level_pixel"]): r for r in acc["rows_outside_1e-3_vs_fp64"]}
        for k in np.nonzero(dl >= 1e-3)[0][:16]:
            rr = ref_rows.get(tuple(int(v) for v in got["ids"][gi[k]]), {})
            tot["rows_outside_1e-3"].append({"seed": seed, "laf_err_px": float(dl[k]), "frame_scale_px": float(S[k]), "rel_err": float(dl[k] / max(S[k], 1e-30)),
                                             "orinet_norm": None if on is None else float(on[k]), "gpu_vs_fp64_px": rr.get("gpu_vs_fp64_px"),
                                             "cpu_vs_fp64_px": rr.get("cpu_vs_fp64_px"), "beyond_referee": rr.get("beyond_referee")})
        tot["images"] += 1
        tot["seeds"].append(seed)
        tot["keypoints"] += len(kw)
        tot["matched"] += len(gi)
        tot["laf_max_px"] = max(tot["laf_max_px"], float(dl.max()))
        tot["laf_rows_within_1e-3"] += int((dl < 1e-3).sum())
        tot["desc_max"] = max(tot["desc_max"], float(dd.max()))
        tot["desc_rows_within_1e-3"] += int((dd < 1e-3).sum())
        tot["responses_equal"] &= bool(np.array_equal(got["resp"][gi], want["resp"][wi]))
        tot["same_row_order"] &= bool(len(gi) == len(kw) and np.array_equal(gi, wi))
    tot["match_rate"] = tot["matched"] / max(tot["keypoints"], 1)
    tot["beyond_budget"] = rf.beyond_budget(tot["matched"])
    tot["golden"] = golden_check(fetch, golden_batch) if golden_batch else None
    tot["pass"] = bool(tot["match_rate"] >= 0.995 and tot["laf_rows_within_1e-3"] >= 0.995 * tot["matched"] and tot["rows_outside_1e-2"] == 0 and
                       tot["rows_outside_5e-3_unexplained"] == 0 and tot["unmatched_unexplained"] == 0 and
                       tot["rows_outside_1e-3_beyond_referee"] <= tot["beyond_budget"] and
                       tot["desc_rows_within_1e-3"] >= 0.995 * tot["matched"] and tot["responses_equal"] and
                       (tot["golden"] is None or tot["golden"]["pass"]))
    tot["bar"] = ("golden leg: see golden.bar.  Live-oracle leg - keys: every key only one side returns traced to a borderline shape-filter decision or the shifted top-N cut "
                  "(unmatched_unexplained = 0); LAF rows: >= 99.5 % within 1e-3 px, NONE outside 1e-2 px, none outside 5e-3 px unless the CPU reference's own row is that far from "
                  "float64; rows outside 1e-3 px that are neither (a) within the CPU reference's own distance to the float64 referee + 1e-3 px nor (b) on a reference row itself >= 1e-3 px "
                  "from fp64 and within 4x its error: at most 1 per 4000 matched rows (budget fixed in oracle/fp64_referee.py before any run); descriptors >= 99.5 % within 1e-3; responses bit-equal")
    tot["reference"] = "oracle/affnet_oracle.py (bit-identical to the unmodified reference, oracle/check_restatement.py) run live on this host; referee oracle/fp64_referee.py"
    torch.set_num_threads(threads_before)
    return tot


DUMP_BYTES = {"rows": 24 << 20, "descriptors": 32 << 20}     # --dump-outputs: beyond these sizes a seeded sample of whole images


def dump_outputs(results, out_dir):
    """--dump-outputs: the rows the last timed step returned to its caller (one dict per fused call: capacity-sized device tensors + row
    counts), images in step order, rows past an image's count set to NaN.  counts (B,); ids (n, NKP, 3) as float64, LAFs (n, NKP, 2, 3) and
    responses (n, NKP) of the images row_images (n,); descriptors (m, NKP, 128) of the images descriptor_images (m,).  Each image set is every
    image while it fits its DUMP_BYTES budget, else a fixed seeded sample (the 64-image step: all rows, descriptors of 32 images), so that
    the files stay below 64 MB together."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    batched = lambda r, k: r[k] if r["count"].numel() > 1 else r[k].unsqueeze(0)
    where = [(r, b) for r in results for b in range(r["count"].numel())]            # image i of the step -> (call, index in that call)
    counts = np.array([int(r["count"].view(-1)[b]) for r, b in where], dtype=np.int64)
    B = len(where)

    def images(per_image, budget):
        n = int(min(B, max(1, budget // per_image)))
        return np.arange(B) if n == B else np.sort(np.random.default_rng(0).choice(B, n, replace=False))

    def rows(key, pick, dt):
        a = np.stack([batched(where[i][0], key)[where[i][1], :NKP].cpu().numpy() for i in pick]).astype(dt)
        a[np.arange(NKP)[None, :] >= counts[pick][:, None]] = np.nan
        return a
    pick = images(NKP * (3 * 8 + 6 * 4 + 4), DUMP_BYTES["rows"])
    arrays = {"counts": counts.astype(np.float64), "row_images": pick.astype(np.float64), "ids": rows("ids", pick, np.float64),
              "lafs": rows("LAFs", pick, np.float32), "responses": rows("responses", pick, np.float32)}
    if results[0]["descriptors"] is not None:
        pick = images(NKP * 128 * 4, DUMP_BYTES["descriptors"])
        arrays.update(descriptor_images=pick.astype(np.float64), descriptors=rows("descriptors", pick, np.float32))
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ----------------------------------------------------------------------------------------------------------------------
LINE_LIMIT = 4096                  # bytes of the ONE stdout line (the driver could not parse a 31 KB line)
DETAIL_FILE = "bench_detail.json"


def _num(v, digits=6):
    """Numbers of the compact line at 6 significant digits (the detail file keeps every digit)."""
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    if isinstance(v, float):
        return float("%.*g" % (digits, v))
    if isinstance(v, dict):
        return {k: _num(x, digits) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_num(x, digits) for x in v]
    return v


def compact_line(d):
    """The ONE line the driver parses, from the full record `d`: the contract's keys + `roofline` + `cpu_baseline` + a handful of scalars per
    co-reported section.  Everything else (stage tables, unmatched-key dossiers, secondary rooflines, gpu_state, exchange details) is in
    bench_detail.json / on stderr.  Never longer than LINE_LIMIT bytes."""
    pick = lambda src, keys: {k: src[k] for k in keys if k in src} if isinstance(src, dict) else None
    line = {k: d.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    cfg = d.get("config", {})
    line["config"] = pick(cfg, ("workload", "global_batch", "keypoints_per_image", "images_per_launch", "parallelism", "keypoints"))
    if isinstance(line["config"].get("workload"), str) and len(line["config"]["workload"]) > 330:
        line["config"]["workload"] = line["config"]["workload"][:327] + "..."
    if "roofline" in d:
        line["roofline"] = pick(d["roofline"], ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "launch_ms", "flops_per_launch"))
        if isinstance(line["roofline"].get("kernel"), str):
            line["roofline"]["kernel"] = line["roofline"]["kernel"][:96]
    cb = d.get("cpu_baseline")
    if isinstance(cb, dict):
        line["cpu_baseline"] = pick(cb, ("value", "unit", "cores", "kind"))
        line["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:150]
        nt = cb.get("node_throughput") or {}
        line["cpu_baseline"]["node_value"] = nt.get("value")
        line["cpu_baseline"]["node_cores"] = nt.get("cores")
    pc = d.get("parity_check")
    if isinstance(pc, dict):
        line["parity"] = pick(pc, ("pass", "images", "keypoints", "matched", "laf_rows_within_1e-3", "laf_max_px", "desc_max", "responses_equal", "unmatched_keys",
                                   "unmatched_unexplained", "rows_outside_1e-3_beyond_referee", "beyond_budget", "rows_outside_1e-2"))
        if isinstance(pc.get("golden"), dict):
            line["parity"]["golden"] = pick(pc["golden"], ("pass", "seeds", "rows", "matched", "rows_outside_1e-3", "laf_max_px", "desc_max"))
    oc = d.get("other_configs")
    other = {}
    if isinstance(oc, dict):
        other.update(pick(oc, ("config2_graph_ms", "config2_eager_ms", "config2_graph_identical_to_eager", "config2_launches", "config5_kp_s", "error")))
        if isinstance(oc.get("config5_roofline"), dict):
            other["config5_frac"] = oc["config5_roofline"].get("frac")
        if isinstance(oc.get("config5_golden"), dict):
            other["config5_golden_pass"] = oc["config5_golden"].get("pass")
            other["config5_golden_rows_outside_1e-3"] = oc["config5_golden"].get("rows_outside_1e-3")
        if isinstance(oc.get("config5_cpu_baseline"), dict):
            other["config5_cpu_kp_s"] = oc["config5_cpu_baseline"].get("value")
    for mode in SPLIT:
        m = d.get("arith_" + mode)
        if isinstance(m, dict):
            short = mode.replace("fp32_", "")
            other[short + "_value"] = m.get("value", m.get("error"))
            if isinstance(m.get("roofline"), dict):
                other[short + "_frac_of_16bit_peak"] = m["roofline"].get("frac")
            if isinstance(m.get("parity_check"), dict):
                other[short + "_parity_pass"] = m["parity_check"].get("pass")
    if other:
        line["other"] = other
    for k in ("affnet_tflops", "orinet_tflops", "all_cnn_tflops"):
        if k in d.get("roofline", {}):
            line.setdefault("cnn", {})[k] = d["roofline"][k]
    if "stage_ms_per_image" in d:
        line["stage_ms_per_image"] = d["stage_ms_per_image"]
    if "ms_per_image" in d:
        line["ms_per_image"] = d["ms_per_image"]
    if d.get("n_gpus", 1) > 1 or "exchange" in d:
        ex = d.get("exchange") or {}
        line["exchange"] = {"mode": ex.get("mode"), "bytes_per_step": ex.get("exchange_bytes_per_step"), "gather_ms": ex.get("gather_ms")}
        pr = d.get("ms_per_step_per_rank") or {}
        line["ms_per_step_per_rank"] = {"min": pr.get("min"), "max": pr.get("max")}
        if isinstance(d.get("gather_check"), dict):
            line["gather_check"] = pick(d["gather_check"], ("identical", "checked", "records", "mode", "error"))
    for k in ("hip_graph", "cold_ms", "warm_ms_min", "dry_run", "records_in_global_order"):          # --config2 / --dry-run lines
        if k in d:
            line[k] = pick(d[k], ("warm_ms", "warm_ms_min", "identical_to_eager", "launches", "error")) if isinstance(d[k], dict) else d[k]
    if isinstance(d.get("wall_s"), dict):
        line["wall_s"] = d["wall_s"].get("total_since_process_start_s")
    line["detail"] = DETAIL_FILE
    line = _num(line)
    text = json.dumps(line, separators=(",", ":"))
    for drop in ("stage_ms_per_image", "cnn", "wall_s", "gather_check", "other", "parity"):          # cannot happen with today's fields; the limit holds regardless
        if len(text) <= LINE_LIMIT:
            break
        line.pop(drop, None)
        text = json.dumps(line, separators=(",", ":"))
    assert len(text) <= LINE_LIMIT, "compact bench line is %d bytes" % len(text)
    return text


def emit(d):
    """Full record -> bench_detail.json (next to bench.py, and gpurun_out/ when present) + stderr; compact line -> stdout, LAST."""
    full = json.dumps(d)
    for path in (os.path.join(ROOT, DETAIL_FILE), os.path.join(ROOT, "gpurun_out", DETAIL_FILE)):
        try:
            if os.path.isdir(os.path.dirname(path)):
                with open(path, "w") as f:
                    f.write(full + "\n")
        except OSError as e:
            sys.stderr.write("bench.py: could not write %s: %r\n" % (path, e))
    sys.stderr.write("bench.py detail record (also in %s):\n%s\n" % (DETAIL_FILE, full))
    sys.stderr.flush()
    try:                               # whatever C libraries have buffered for stdout (RCCL's version banner: seen AFTER the line in a file) goes out first
        C.CDLL(None).fflush(None)
    except Exception:                  # noqa: BLE001
        pass
    sys.stdout.flush()
    print(compact_line(d), flush=True)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_spawn(args):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script (one per device), relay their output,
    fail loudly if fewer devices exist or any rank fails.  Rank 0 prints the one JSON line."""
    n = args.gpus
    one_device = bool(os.environ.get("AFFNET_BENCH_ONE_DEVICE"))
    if not args.dry_run:
        have = torch.cuda.device_count()
        if have < n and not one_device:
            sys.stderr.write("bench.py: --gpus %d needs %d visible GPUs, found %d (set AFFNET_BENCH_ONE_DEVICE=1 only for a "
                             "single-device dry run of the multi-rank path)\n" % (n, n, have))
            return 2
    env = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0",
               AFFNET_BENCH_SPAWNED="1")
    procs = []
    for r in range(n):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=e))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in pending:              # one rank failed: the others would hang in the next collective
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if rc != 0:
        sys.stderr.write("bench.py: a rank exited with code %d - no result\n" % rc)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=BATCH, help="images per step per rank")
    ap.add_argument("--chunk", type=int, default=int(os.environ.get("AFFNET_BENCH_CHUNK", "32")),
                    help="images per fused library call (every kernel launch covers `chunk` images)")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("AFFNET_BENCH_STREAMS", "1")),
                    help="independent streams (each with its own context) the chunks alternate over")
    ap.add_argument("--pipeline", type=int, default=int(os.environ.get("AFFNET_BENCH_PIPELINE", "0")),
                    help="1 (with --streams 1): pyramid + detector of chunk i+1 run on a second stream next to the CNN stages of "
                         "chunk i (two contexts alternate); the CNN kernels stay serialised on one stream")
    ap.add_argument("--gather", choices=("all", "rank0"), default="rank0",
                    help="N > 1 exchange of the padded records: gather to rank 0 (default; what north_star names: 69 MB out of every other rank, "
                         "484 MB into rank 0 per 64-image step at N = 8) or all_gather (every rank receives the 484 MB: 8x the xGMI traffic)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the stand-alone sampler timing behind secondary_rooflines")
    ap.add_argument("--include-h2d", action="store_true",
                    help="every step's images come from pinned host memory: uploaded on a copy stream into a double-buffered device "
                         "buffer while the previous step computes (a separately labelled, PCIe-inclusive line - never the headline value)")
    ap.add_argument("--config2", action="store_true",
                    help="BASELINE.json configs[1]: latency of ONE image (tests/golden/graf_img1.png = test-graf/img1.png, 2000 kp, "
                         "B = 1), pinned host -> device upload included; cold (context creation) and warm")
    ap.add_argument("--config5", action="store_true",
                    help="BASELINE.json configs[4] instead of the headline configs[2]: 3840x2160 images, 8000 kp each (deep pyramid stress); "
                         "batch / chunk default to 8 / 8")
    ap.add_argument("--all-candidates", action="store_true",
                    help="run AffNet on all 1.5 N candidates at once like the reference (affnet_config.lazy_shape_rows = 0) instead of the default "
                         "lazy evaluation (first 1.2 N response-sorted candidates, the rest only for images that still lack N survivors of the "
                         "shape filter; output rows are identical either way)")
    ap.add_argument("--onepass", action="store_true",
                    help="OnePassSIR path (SURVEY section 8f row 4) instead of the headline path: affine shapes from ONE dense AffNetFastFullConv "
                         "evaluation per octave (shipped AffNet.pth weights), border = 15 like the reference's scripts; a separately labelled line")
    ap.add_argument("--verify-gather", nargs="?", const="all", default=None, metavar="all|sample|off",
                    help="after the timed region rank 0 re-computes gathered records of the LAST step itself (single-image calls on the same "
                         "seeds) and compares them bit for bit with what arrived through the exchange: right content, count and global order. "
                         "Default for N > 1: 'sample' (first and last image of every rank); 'all' checks every record; N = 1 with "
                         "AFFNET_BENCH_SELF_GATHER=1 checks the 1-rank RCCL path")
    ap.add_argument("--arith", choices=("fp32", "fp32_split3", "fp32_split2h"), default="fp32",
                    help="arithmetic of the CNN contractions (include/affnet_hip.h AFFNET_ARITH_*): fp32 = exact fp32 MFMA (default, the headline "
                         "`value`); fp32_split3 = fp32 operands as three bf16 terms (six products) on the bf16 matrix cores, fp32_split2h = two fp16 "
                         "terms (three products) on the fp16 matrix cores, fp32 accumulate - separately labelled lines with their own roofline "
                         "against the bf16 / fp16 peak")
    ap.add_argument("--split3", action="store_true", help="same as --arith fp32_split3")
    ap.add_argument("--no-split3", action="store_true", help="skip the co-reported `arith_fp32_split3` / `arith_fp32_split2h` steps of the default line")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short BASELINE configs[1] (single-image latency) and configs[4] (4K) samples behind `other_configs`")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the CPU baseline and parity_check, the co-reported arithmetic modes, "
                         "other_configs, secondary_rooflines, the stand-alone exchange timing and gather check of the N-rank path, gpu_state "
                         "(the --no-* options above drop single parts of it).  Without it a run sets up, warms up, times --steps steps, "
                         "writes --dump-outputs and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step returned (rank 0's images) as DIR/<name>.npy, "
                         "float32 / float64, at most 64 MB (see dump_outputs)")
    ap.add_argument("--cpu-worker", default=None, help=argparse.SUPPRESS)        # child process of cpu_node_throughput()
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU work: ranks rendezvous (backend from AFFNET_BENCH_BACKEND, default gloo here), exchange fake records and "
                         "print the JSON skeleton - exercises the launch / world-size / gather bookkeeping on a CPU host")
    args = ap.parse_args()
    if args.split3:
        args.arith = "fp32_split3"
    args.split3 = args.arith in SPLIT          # a split-operand mode is the line's arithmetic
    if args.cpu_worker:
        return cpu_worker(args.cpu_worker)
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_spawn(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and not os.environ.get("AFFNET_BENCH_SELF_GATHER"):
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d: refusing to report a run whose n_gpus would be wrong\n" % (args.gpus, world))
        sys.exit(2)
    if args.config2:
        return config2_latency(args)
    run(args, world)


# ----------------------------------------------------------------------------------------------------------------------
def config2_latency(args):
    """BASELINE configs[1] (hesaffnet.py:35-60 on test-graf/img1.png, 2000 kp): what a caller of the single-image API
    waits for.  Cold = first call of a fresh process state (context + workspace creation, weight packing + upload, module
    load); warm = median of the following calls; both include the pinned-host -> device upload of the image."""
    import numpy as np
    from PIL import Image
    import affnet_amd
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    img = np.mean(np.array(Image.open(GRAF).convert("RGB")), axis=2).astype(np.float32)          # hesaffnet.py:35-36
    host = torch.from_numpy(img).view(1, 1, img.shape[0], img.shape[1]).pin_memory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    A = affnet_amd.AffNetFast(PS=32)
    A.load_state_dict(torch.load(os.path.join(ROOT, "pretrained", "AffNet.pth"), map_location="cpu", weights_only=False)["state_dict"])
    O = affnet_amd.OriNetFast(PS=32)
    O.load_state_dict(torch.load(os.path.join(ROOT, "pretrained", "OriNet.pth"), map_location="cpu", weights_only=False)["state_dict"])
    Hn = affnet_amd.HardNet()
    Hn.load_state_dict(affnet_amd.synthetic_hardnet_state(0))
    A, O, Hn = A.to(dev), O.to(dev), Hn.to(dev)
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=2000, border=5, num_Baum_iters=1, AffNet=A, OriNet=O, arith=args.arith).to(dev)
    x = host.to(dev, non_blocking=True)
    r = det.run(x, do_ori=True, desc=Hn)
    torch.cuda.synchronize()
    cold = time.perf_counter() - t0
    out = config2_measure(det, Hn, host, dev, max(args.steps, 5) * 4, args.arith)
    out["cold_ms"] = cold * 1e3
    out["note"] = "cold = weight load + BN folding + packing + upload, context / workspace creation, HIP module load and the first call"
    emit(out)


def config2_measure(det, Hn, host, dev, n_lat, arith):
    """Warm single-image latency of `det` on the pinned host image `host` (eager calls, then the same call replayed as one HIP graph)."""
    split3 = arith in SPLIT
    x = host.to(dev, non_blocking=True)
    r = det.run(x, do_ori=True, desc=Hn)
    torch.cuda.synchronize()
    n = int(r["LAFs"].shape[0])
    lat = []
    for _ in range(n_lat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = host.to(dev, non_blocking=True)
        r = det.run(x, do_ori=True, desc=Hn)            # includes the one count read-back (= a stream sync)
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    lat.sort()
    warm = lat[len(lat) // 2]
    # the same call replayed as ONE HIP graph (affnet_graph_capture_extract): ~45 launches per image become one
    glat, gerr = [], None
    try:
        cap = det.capture(x, do_ori=True, desc=Hn)
        for i in range(len(lat) + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cap.image.copy_(host, non_blocking=True)           # pinned host -> the captured input buffer
            r2 = cap.run(check_weights=(i == 0))               # frozen weights: the per-replay stamp walk (~50 us of Python) only once
            torch.cuda.synchronize()
            if i >= 3:
                glat.append(time.perf_counter() - t0)
        same = all(torch.equal(r[k], r2[k]) for k in ("LAFs", "responses", "descriptors"))
        glat.sort()
    except Exception as e:                                      # noqa: BLE001  (reported in the line, the eager figures stand)
        gerr, same = repr(e), False
    out = {"metric": "latency per image (hesaffnet.py test-graf/img1.png, 2000 kp, detect+AffNet+OriNet+HardNet, B=1, H2D included)" +
                     (" [arith %s: %s]" % (arith, SPLIT[arith]["label"]) if split3 else ""),
           "value": warm * 1e3, "unit": "ms", "n_gpus": 1, "steps": len(lat), "warmup": 1, "ms_per_step": warm * 1e3,
           "higher_is_better": False, "scaling": "weak", "vs_baseline": None,
           "dtype": SPLIT[arith]["dtype"] if split3 else "f32",
           "data": "tests/golden/graf_img1.png (byte copy of test-graf/img1.png)",
           "config": {"workload": "BASELINE.json configs[1]: hesaffnet.py test-graf/img1.png 2000 kp, full path on 1 MI355X, single-image API "
                                  "(ScaleSpaceAffinePatchExtractor.run), %dx%d, pinned host image uploaded inside the timed call" % (host.size(3), host.size(2)),
                      "keypoints": n},
           "warm_ms_min": lat[0] * 1e3, "warm_ms_p90": lat[int(0.9 * len(lat))] * 1e3,
           "keypoints_per_s_warm": n / warm,
           "hip_graph": ({"warm_ms": glat[len(glat) // 2] * 1e3, "warm_ms_min": glat[0] * 1e3, "keypoints_per_s_warm": n / glat[len(glat) // 2],
                          "identical_to_eager": bool(same), "what": "the whole path captured once (affnet_graph_capture_extract) and replayed with a "
                                                                    "single hipGraphLaunch per image; H2D into the captured input buffer included"}
                         if glat else {"error": gerr})}
    return out


# ----------------------------------------------------------------------------------------------------------------------
def run(args, world):
    global H, W, NKP
    if args.config5:
        H, W, NKP = 2160, 3840, 8000
        if args.batch == BATCH:
            args.batch = 8
        if args.chunk == 32:
            args.chunk = 8
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if rank != 0:                      # only rank 0 owns stdout (the ONE line): what the other ranks' libraries print there goes to stderr
        sys.stdout.flush()
        os.dup2(2, 1)
    import torch.distributed as dist
    DRY = args.dry_run
    one_device = bool(os.environ.get("AFFNET_BENCH_ONE_DEVICE"))
    if one_device:
        local_rank = 0
    # AFFNET_BENCH_SELF_GATHER=1 (single process): a 1-rank RCCL group, so that the stream-ordered gather of the N > 1
    # path runs on a 1-GPU box (tools/gpu_dist_dryrun.sh); AFFNET_BENCH_BACKEND=gloo + AFFNET_BENCH_ONE_DEVICE=1: N ranks on one GPU
    SELF = world == 1 and bool(os.environ.get("AFFNET_BENCH_SELF_GATHER"))
    DIST = world > 1 or SELF
    backend = os.environ.get("AFFNET_BENCH_BACKEND", "gloo" if DRY else "nccl")
    if not DRY:
        if local_rank >= torch.cuda.device_count():
            sys.stderr.write("bench.py: rank %d needs device %d but only %d are visible\n" % (rank, local_rank, torch.cuda.device_count()))
            sys.exit(2)
        torch.cuda.set_device(local_rank)
    dev = torch.device("cpu") if DRY else torch.device("cuda", local_rank)
    if DIST:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(backend, rank=rank, world_size=world)
        assert dist.get_world_size() == world == max(args.gpus, 1), "world size %d != --gpus %d" % (dist.get_world_size(), args.gpus)
        # one DISTINCT device per rank (a mis-set LOCAL_RANK / HIP_VISIBLE_DEVICES would otherwise stack ranks on one GPU)
        ident = "cpu-%d" % rank if DRY else "%s|%s" % (getattr(torch.cuda.get_device_properties(local_rank), "uuid", local_rank), local_rank)
        idents = [None] * world
        dist.all_gather_object(idents, ident)
        if len(set(idents)) != world and not one_device:
            sys.stderr.write("bench.py: %d ranks share devices %s - refusing (AFFNET_BENCH_ONE_DEVICE=1 allows it for dry runs)\n" % (world, idents))
            sys.exit(2)
    gather_dst = 0 if args.gather == "rank0" else None

    from affnet_amd import sharded
    if DRY:
        return dry_run(args, world, rank, dist, sharded, DIST, gather_dst, backend)

    import affnet_amd
    from affnet_amd import _lib
    from affnet_amd.synthetic import synthetic_image
    if world > 1:                      # N ranks generate their synthetic images side by side: do not let each of them spin up every core
        torch.set_num_threads(max(1, min(16, host_threads()[1] // world)))

    def load(name, cls):
        net = cls(PS=32) if name != "HardNet" else cls()
        if name != "HardNet":
            net.load_state_dict(torch.load(os.path.join(ROOT, "pretrained", name + ".pth"), map_location="cpu", weights_only=False)["state_dict"])
        else:
            net.load_state_dict(affnet_amd.synthetic_hardnet_state(0))
        return net.to(dev)

    A, O, Hn = load("AffNet", affnet_amd.AffNetFast), load("OriNet", affnet_amd.OriNetFast), load("HardNet", affnet_amd.HardNet)
    ONEPASS = args.onepass
    if ONEPASS:
        FC = affnet_amd.AffNetFastFullConv()
        FC.load_state_dict(torch.load(os.path.join(ROOT, "pretrained", "AffNet.pth"), map_location="cpu", weights_only=False)["state_dict"])
        FC = FC.to(dev)
    # global image i of a step lives on rank i % world (weak scaling: `batch` images per rank per step)
    seeds = [rank + world * j for j in range(args.batch)]
    CH = max(1, min(args.chunk, args.batch))
    host_imgs = torch.cat([synthetic_image(H, W, s) for s in seeds], 0)
    H2D = args.include_h2d
    if H2D:
        host_imgs = host_imgs.pin_memory()
        dev_bufs = [torch.empty_like(host_imgs, device=dev) for _ in range(2)]      # double buffer: upload k+1 while k computes
        copy_stream = torch.cuda.Stream(device=dev)
        imgs = dev_bufs[0]
    else:
        imgs = host_imgs.to(dev)                                                       # (batch,1,H,W) resident in HBM
    n_chunks = (args.batch + CH - 1) // CH
    chunk_of = lambda buf: [buf[i:i + CH] for i in range(0, args.batch, CH)]
    chunks = chunk_of(imgs)
    S = max(1, args.streams)
    PIPE = bool(args.pipeline) and S == 1
    if PIPE:
        S = 2                          # two contexts alternate; ONE CNN stream + ONE detector stream
    # one extractor (context + workspace) per (stream, chunk size); a ragged last chunk gets its own
    dets = {}
    for ci, c in enumerate(chunks):
        k = (ci % S, c.size(0))
        if k not in dets and ONEPASS:
            dets[k] = affnet_amd.OnePassSIR(mrSize=5.192, num_features=NKP, border=15, num_Baum_iters=1, AffNet=FC, OriNet=O, arith=args.arith).to(dev)
            dets[k]._context(c)
        if k not in dets:
            dets[k] = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=NKP, border=5, num_Baum_iters=1,
                                                                AffNet=A, OriNet=O, arith=args.arith).to(dev)
            if args.all_candidates:
                dets[k].lazy_shape_rows = 0
            elif os.environ.get("AFFNET_BENCH_LAZY_ROWS"):              # tuning aid: size of the first AffNet pass (default N + N / 5; same output rows for any value)
                dets[k].lazy_shape_rows = int(os.environ["AFFNET_BENCH_LAZY_ROWS"])
            dets[k]._context(c, allow_batch=True)  # create contexts / workspaces before anything is timed
    streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
    det_stream = torch.cuda.Stream(device=dev) if PIPE else None

    pending = [None]                   # finish() of the previous step's gather (overlaps with this step's compute)
    # Steps are enqueued back to back; nothing inside the timed region waits on the host (the keypoint counts are
    # summed on the device and read once after the closing synchronize, the RCCL gather of step k is ordered behind
    # step k's kernels by stream semantics and waited for, on the stream, in step k+1).  A host-side sync + count
    # read-back per step left the GPU idle ~2.4 ms per 135 ms step while the host launched the next step's detector.
    LAZY = not PIPE and S == 1 and not (DIST and dist.get_backend() != "nccl")
    kp_dev = torch.zeros((), dtype=torch.int64, device=dev)
    ovf_dev = torch.zeros((), dtype=torch.int64, device=dev)     # capacity-overflow flags of EVERY step, accumulated on the device
    inflight = []
    step_no = [0]
    upload_done = [None, None]         # events: buffer b holds the images of its step
    compute_done = [None, None]        # events: the step that read buffer b has finished (buffer may be overwritten)

    def upload(b):
        with torch.cuda.stream(copy_stream):
            if compute_done[b] is not None:
                copy_stream.wait_event(compute_done[b])
            dev_bufs[b].copy_(host_imgs, non_blocking=True)
            upload_done[b] = torch.cuda.Event()
            upload_done[b].record(copy_stream)

    def step():
        cur_chunks = chunks
        b = step_no[0] & 1
        if H2D:
            if upload_done[b] is None:
                upload(b)                                       # first step: nothing to overlap with
            cur_chunks = chunk_of(dev_bufs[b])
            for s in streams:
                s.wait_event(upload_done[b])
            upload_done[b] = None
            upload(b ^ 1)                                       # next step's images travel while this step computes
        results = [None] * len(cur_chunks)
        for ci, c in enumerate(cur_chunks):
            with torch.cuda.stream(streams[0] if PIPE else streams[ci % S]):
                if ONEPASS:
                    results[ci] = dets[(ci % S, c.size(0))].enqueue(c, do_ori=True, desc=Hn)
                else:
                    results[ci] = dets[(ci % S, c.size(0))].enqueue(c, do_ori=True, desc=Hn, det_stream=det_stream, input_ready=False)
        step_no[0] += 1
        if LAZY:
            with torch.cuda.stream(streams[0]):
                if len(inflight) >= 2:
                    inflight.pop(0).synchronize()               # host stays at most two steps ahead of the GPU (bounds memory)
                kp_dev.add_(torch.stack([r["count"].sum() for r in results]).sum())
                ovf_dev.add_(torch.stack([r["overflow"].ne(0).sum() for r in results]).sum())
                if DIST:
                    if pending[0] is not None:
                        pending[0]()                            # stream-side wait for the previous step's gather
                    pending[0] = sharded.gather_features_async(sharded.pack_batched_records(results, NKP), args.batch * world, force=SELF,
                                                               dst=gather_dst)
                ev = torch.cuda.Event()
                ev.record()
                inflight.append(ev)
                if H2D:
                    compute_done[b] = ev
            return results
        for s in streams:
            s.synchronize()
        kp_dev.add_(sum(int(r["count"].sum().item()) for r in results))
        ovf_dev.add_(sum(int(r["overflow"].ne(0).sum().item()) for r in results))
        if H2D:
            compute_done[b] = None
        if DIST:
            if pending[0] is not None:
                pending[0]()                                    # records of the previous step have arrived
            rec = sharded.pack_batched_records(results, NKP)
            torch.cuda.synchronize()
            pending[0] = sharded.gather_features_async(rec, args.batch * world, force=SELF, dst=gather_dst)
        return results

    gathered = [None]                  # records of the last drained step in global image order (None on ranks a rank-0 gather skips)

    def drain():
        if pending[0] is not None:
            with torch.cuda.stream(streams[0]):
                gathered[0] = pending[0]()
            pending[0] = None
        torch.cuda.synchronize()

    def barrier():
        if DIST:
            if dist.get_backend() == "nccl":
                dist.barrier(device_ids=[local_rank])
            else:
                dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    drain()
    for d in dets.values():
        _lib.check(_lib.lib.affnet_profile_enable(d._ctx.handle, 1), d._ctx.handle, "profile_enable")
    kp_dev.zero_()
    ovf_dev.zero_()
    barrier()
    gpu_sections = []                  # wall-clock (unix seconds) start / end of every GPU section of this run: lets an outside sampler (rocm-smi) be lined up
    wall = {"setup_and_warmup_s": round(time.time() - T_START, 1)}      # imports of this package, synthetic images, weights, contexts, warm-up steps
    w0 = time.time()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = step()
    drain()                            # every step's kernels and the last gather complete inside the timed region
    barrier()
    dt = time.perf_counter() - t0
    gpu_sections.append({"what": "timed region (%d steps)" % args.steps, "unix_start_s": w0, "unix_end_s": time.time()})
    if args.dump_outputs and rank == 0:
        dump_outputs(last, args.dump_outputs)
    smi = gpu_state("right after the timed region") if (args.full and rank == 0 and not DIST) else None
    kp = int(kp_dev.item())
    # a list that overflowed would have truncated the keypoint set the rate is computed on: fail instead of reporting it.  The
    # per-image flags are cleared at the start of every call, so they are summed on the device after each step (the contexts' own
    # read-back below only sees their last call)
    if int(ovf_dev.item()) != 0:
        sys.stderr.write("bench.py: a fixed-capacity detector list overflowed in %d image(s) of the timed steps: rows were truncated\n" % int(ovf_dev.item()))
        sys.exit(4)
    for d in dets.values():
        d._ctx.read_counts(allow_empty=True)
    # candidates AffNet was actually evaluated on (lazy shape evaluation: ~1.2 N instead of 1.5 N per image), from the device counters
    # of every context's last call; the FLOP rates below use it
    aff_eval = []
    if not ONEPASS:
        for d in dets.values():
            aff_eval += d._ctx.counter_view(3).cpu().tolist()
    aff_eval_per_img = (sum(aff_eval) / len(aff_eval)) if aff_eval else 0.0
    # stage timings recorded by HIP events on the launch streams during the timed region
    def read_profile(keep_on=False):
        sums, calls, call_imgs = [0.0] * 8, 0, 0
        for (_, nimg), d in dets.items():
            buf, n = (C.c_double * 8)(), C.c_int32(0)
            _lib.check(_lib.lib.affnet_profile_read(d._ctx.handle, C.byref(buf), C.byref(n)), d._ctx.handle, "profile_read")
            if not keep_on:
                _lib.check(_lib.lib.affnet_profile_enable(d._ctx.handle, 0), d._ctx.handle, "profile_enable")
            calls += n.value
            call_imgs += n.value * nimg
            sums = [a + b for a, b in zip(sums, list(buf))]
        return sums, calls, call_imgs
    sums, calls, call_imgs = read_profile(keep_on=True)
    t_all = torch.tensor([dt], dtype=torch.float64, device=dev)
    kp_all = torch.tensor([kp], dtype=torch.float64, device=dev)
    rank_ms = [dt / args.steps * 1e3]
    if world > 1:
        per_rank = [torch.zeros_like(t_all) for _ in range(world)]
        dist.all_gather(per_rank, t_all)
        rank_ms = [float(t.item()) / args.steps * 1e3 for t in per_rank]
        dist.all_reduce(t_all, op=dist.ReduceOp.MAX)
        dist.all_reduce(kp_all, op=dist.ReduceOp.SUM)
    # ---- the exchange on its own (outside the timed region): bytes, stand-alone duration, and the content check ----------------------
    exchange = None
    if DIST and args.full:
        rec_local = sharded.pack_batched_records(last, NKP)                      # this rank's records of the last step
        times = []
        for _ in range(5):
            barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fin = sharded.gather_features_async(rec_local, args.batch * world, force=SELF, dst=gather_dst)
            got = fin()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        rec_bytes = int(rec_local.size(1)) * 4
        exchange = {"mode": "all_gather" if gather_dst is None else "gather_rank0", "record_bytes": rec_bytes, "records_per_step": args.batch * world,
                    "exchange_bytes_per_step": rec_bytes * args.batch * world * (world if gather_dst is None else 1),
                    "what": "all_gather: every rank receives every record" if gather_dst is None else "gather: rank 0 receives every record",
                    "gather_ms": times[len(times) // 2], "gather_ms_min": times[0],
                    "how": "median of 5 stand-alone exchanges of one step's records after the timed region (HIP events around issue + wait, "
                           "barrier first); inside the timed region the exchange of step k runs under the kernels of step k+1"}
        if SELF and world == 1:
            # the record volume of ONE step at N = 8 (8 x 64 records = 553 MB at 2000 kp) through the same call in the 1-rank RCCL group: the
            # software floor (pack, enqueue, local copy) the first real 8-GPU line's gather_ms can be read against - no xGMI link is crossed here
            rec8 = rec_local.repeat(8, 1)
            t8 = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sharded.gather_features_async(rec8, args.batch * 8, force=True, dst=gather_dst)()
                e1.record()
                torch.cuda.synchronize()
                t8.append(e0.elapsed_time(e1))
            t8.sort()
            exchange["n8_volume_1rank"] = {"records": int(rec8.size(0)), "bytes": int(rec8.numel()) * 4, "gather_ms": t8[len(t8) // 2], "gather_ms_min": t8[0],
                                           "note": "one rank, no link crossed: software floor of the exchange at the N = 8 record volume"}
            del rec8
    mode = args.verify_gather or ("sample" if args.full and DIST else "off")
    gather_check = None
    if DIST and mode != "off":
        gather_check = verify_gather(gathered[0], mode, world, rank, args.batch, dev, (A, O, Hn), ONEPASS)
    if rank == 0:
        tmax, kps = float(t_all.item()), float(kp_all.item())
        stage_ms = [s / max(call_imgs, 1) for s in sums]           # per image (rank 0's launches)
        names = ["pyramid", "detector", "affnet", "shape_filter", "orinet", "denorm_levelsel", "hardnet_trunk", "hardnet_head"]
        img_per_launch = call_imgs / max(calls, 1)
        trunk_ms = sums[6] / max(calls, 1)                          # mean duration of one HardNet trunk launch
        kp_per_img = kps / max(1, args.steps * args.batch * world)
        flops_launch = kp_per_img * img_per_launch * (FLOP_HARD - FLOP_HARD_HEAD)
        achieved = flops_launch / (trunk_ms * 1e-3) / 1e12 if trunk_ms > 0 else 0.0
        traffic, traffic_note = pmc_traffic(img_per_launch, split=args.arith if args.split3 else False)
        cfg_idx = 4 if args.config5 else 2
        metric = "keypoints/sec (detect+AffNet+OriNet+HardNet) per image, %d kp @%dx%d" % (NKP, W, H)
        if H2D:
            metric += " [PCIe-inclusive: images uploaded from pinned host memory every step]"
        if args.split3:
            metric += " [arith %s: %s]" % (args.arith, SPLIT[args.arith]["label"])
        if ONEPASS:
            metric = "keypoints/sec (OnePassSIR: detect + dense AffNetFastFullConv per octave + OriNet + HardNet) per image, %d kp @%dx%d" % (NKP, W, H)
        out = {
            "metric": metric,
            "value": kps / tmax, "unit": "keypoints/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": tmax / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": SPLIT[args.arith]["dtype"] if args.split3 else "f32", "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[%d]: batch of %d synthetic %dx%d grayscale images per GPU per step, "
                                   "%d kp each, full path detect+AffNet+OriNet+HardNet; AffNet/OriNet shipped weights, "
                                   "HardNet seeded synthetic weights (HardNet++.pth is a missing blob)%s"
                                   % (cfg_idx, args.batch, W, H, NKP,
                                      " = BASELINE.json configs[3] (512-image stream, image-per-GPU over 8 GPUs) per step" if world == 8 and not args.config5 else ""),
                       "global_batch": args.batch * world, "keypoints_per_image": kp_per_img,
                       "affnet_evaluation": ("all %d candidates per image at once (like the reference)" % int(1.5 * NKP)) if args.all_candidates else
                                            ("lazy: the first %d of the %d response-sorted candidates, the rest only for images that lack %d survivors "
                                             "of the shape filter (device-side decision; output rows identical to the all-at-once evaluation); "
                                             "evaluated per image: %.0f" % (NKP + (NKP + 4) // 5, int(1.5 * NKP), NKP, aff_eval_per_img)),
                       "images_per_launch": CH,
                       "streams_per_gpu": "1 CNN stream + 1 detector stream (2 contexts alternate)" if PIPE else S,
                       "h2d": "every step uploads its images from pinned host memory on a copy stream (double-buffered)" if H2D
                              else "images resident in HBM before the timed region",
                       "parallelism": ("image-per-GPU x%d, %s of padded {int32 count, LAFs, responses, descriptors} records over %s"
                                       % (world, "all_gather" if gather_dst is None else "gather to rank 0",
                                          "RCCL" if backend == "nccl" else backend + " (dry run of the N-rank path)")) if world > 1 else "1 GPU"},
            "ms_per_image": tmax / (args.steps * args.batch) * 1e3,
            "stage_ms_per_image": dict(zip(names, [round(v, 4) for v in stage_ms])),
            "ms_per_step_per_rank": {"min": min(rank_ms), "max": max(rank_ms), "all": [round(v, 3) for v in rank_ms]},
            "roofline": {"kernel": "cnn32_trunk_kernel<HardNet> (fp32 MFMA 16x16x4, fused sampler+norm+6 convs)", "bound": "mfma",
                         "achieved": achieved, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": achieved / PEAK_FP32_MFMA_TFLOPS,
                         "traffic": traffic, "traffic_source": traffic_note, "flops_per_launch": flops_launch, "launch_ms": trunk_ms,
                         "all_cnn_tflops": (aff_eval_per_img * FLOP_AFF + kp_per_img * (FLOP_ORI + FLOP_HARD)) /
                                           (max(stage_ms[2] + stage_ms[4] + stage_ms[6] + stage_ms[7], 1e-9) * 1e-3) / 1e12,
                         "affnet_patches_evaluated_per_image": aff_eval_per_img,
                         "affnet_tflops": aff_eval_per_img * FLOP_AFF / (max(stage_ms[2], 1e-9) * 1e-3) / 1e12,
                         "orinet_tflops": kp_per_img * FLOP_ORI / (max(stage_ms[4], 1e-9) * 1e-3) / 1e12},
        }
        def split_roofline(launch_ms, fl_launch, mode):
            """HardNet trunk on split operands: SIX bf16 / THREE fp16 MFMA products per fp32 product (conv0 stays fp32) - priced against the bf16 = fp16 peak."""
            prod = SPLIT[mode]["products"]
            f_conv0 = kp_per_img * img_per_launch * 2.0 * 1024 * 9 * 32
            bf16_tf = prod * (fl_launch - f_conv0) / (launch_ms * 1e-3) / 1e12 if launch_ms > 0 else 0.0
            eq = fl_launch / (launch_ms * 1e-3) / 1e12 if launch_ms > 0 else 0.0
            tr, tr_note = pmc_traffic(img_per_launch, split=mode)
            return {"kernel": "cnn32_trunk_kernel<HardNet, split operands> (conv1..conv5: %s per fp32 product, fp32 accumulate; conv0 fp32 MFMA)" % SPLIT[mode]["insn"],
                    "bound": "mfma", "achieved": bf16_tf, "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": bf16_tf / PEAK_BF16_MFMA_TFLOPS,
                    "traffic": tr, "traffic_source": tr_note, "flops_per_launch": fl_launch, "launch_ms": launch_ms,
                    "fp32_equivalent_tflops": eq, "fp32_equivalent_vs_fp32_mfma_peak": eq / PEAK_FP32_MFMA_TFLOPS,
                    "note": "executed 16-bit matrix FLOPs (%d per algorithmic fp32 FLOP) against the dense bf16 / fp16 MFMA peak" % int(prod)}
        if args.split3:
            keep = {k: out["roofline"][k] for k in ("all_cnn_tflops", "affnet_patches_evaluated_per_image", "affnet_tflops", "orinet_tflops")}
            out["roofline"] = dict(split_roofline(trunk_ms, flops_launch, args.arith), **keep)
        if exchange is not None:
            out["exchange"] = exchange
        if gather_check is not None:
            out["gather_check"] = gather_check
        if ONEPASS:
            out["stage_ms_per_image"]["detector"] = round(stage_ms[1], 4)
            out["config"]["workload"] = ("OnePassSIR path (SURVEY section 8f row 4) on the BASELINE configs[2] images: batch of %d synthetic %dx%d images, %d kp, "
                                         "border 15; the detector stage includes the dense AffNetFastFullConv of every octave" % (args.batch, W, H, NKP))
        if args.full and not args.no_secondary and not ONEPASS and world == 1:
            out["secondary_rooflines"] = secondary_rooflines(dets, chunks, stage_ms, dev)
        # Co-reported, NOT `value`: the same step in the other arithmetic mode of the boundary (AFFNET_ARITH_FP32_SPLIT3: every CNN contraction
        # on split operands, fp32 = three bf16 terms on the bf16 matrix cores, fp32 accumulate) - a few steps on the same contexts after
        # the timed region, with its own stage events, roofline (bf16 peak), dtype and parity_check
        last_split = {}
        if args.full and world == 1 and not ONEPASS and not args.split3 and not args.no_split3:
            for mode in SPLIT:
                key = "arith_" + mode
                try:
                    for d in dets.values():
                        d.arith = mode                                   # the extractor switches its context on the next call (same buffers)
                    n3 = 8
                    step(); step(); drain()
                    read_profile(keep_on=True)                           # discard the warm-up steps' events
                    kp_dev.zero_()
                    torch.cuda.synchronize()
                    w1, t1 = time.time(), time.perf_counter()
                    for _ in range(n3):
                        last_split[mode] = step()
                    drain()
                    dt3 = time.perf_counter() - t1
                    gpu_sections.append({"what": "%s (%d steps)" % (key, n3), "unix_start_s": w1, "unix_end_s": time.time()})
                    s3_sums, s3_calls, s3_imgs = read_profile(keep_on=True)
                    s3_stage = [v / max(s3_imgs, 1) for v in s3_sums]
                    out[key] = {
                        "value": int(kp_dev.item()) / dt3, "unit": "keypoints/s", "steps": n3, "ms_per_image": dt3 / (n3 * args.batch) * 1e3,
                        "dtype": SPLIT[mode]["dtype"], "vs_value": int(kp_dev.item()) / dt3 / (kps / tmax),
                        "stage_ms_per_image": dict(zip(names, [round(v, 4) for v in s3_stage])),
                        "roofline": split_roofline(s3_sums[6] / max(s3_calls, 1), flops_launch, mode),
                        "note": "another arithmetic mode of the boundary (affnet_config.arith / affnet_set_arith), never the headline: fp32 operands as "
                                "%s, %s per product, fp32 accumulate; differs from the default path like one fp32 summation order from another (every "
                                "full-path GPU test runs in all modes with the same bars)"
                                % ("three bf16 terms (exact)" if mode == "fp32_split3" else "two fp16 terms (to 2^-23 relative for |x| >= 2^-2, 2^-25 absolute below)", SPLIT[mode]["insn"])}
                except Exception as e:                                   # noqa: BLE001  (never at the expense of the main line)
                    out[key] = {"error": repr(e)[:300]}
                    last_split.pop(mode, None)
                finally:
                    for d in dets.values():
                        d.arith = args.arith
                        d._ctx.set_arith(args.arith)
        for d in dets.values():
            _lib.lib.affnet_profile_enable(d._ctx.handle, 0)
        # BASELINE configs[1] and configs[4] in the default line (short samples after the timed region; `--config2` / `--config5` are the full runs)
        t_oc = time.time()
        if args.full and world == 1 and not ONEPASS and not args.config5 and not args.no_other_configs and args.batch == BATCH:
            try:
                out["other_configs"] = other_configs((A, O, Hn), dev, args.arith, gpu_sections, with_cpu=not args.no_cpu_baseline)
            except Exception as e:                                   # noqa: BLE001
                out["other_configs"] = {"error": repr(e)[:300]}
        out["gpu_sections_unix_s"] = gpu_sections
        if smi is not None:
            out["gpu_state"] = smi
        wall["other_configs_s"] = round(time.time() - t_oc, 1)          # incl. the one-image 4K CPU baseline
        if args.full and world == 1 and not args.no_cpu_baseline and not args.config5 and not ONEPASS:
            t_cb = time.time()
            base, kept = cpu_baseline()
            out["cpu_baseline"] = base
            wall["cpu_baseline_s"] = round(time.time() - t_cb, 1)

            def fetcher(results):
                def fetch(seed):                                     # image `seed` of a step (rank 0, world 1: seed == index)
                    r = results[seed // CH]
                    b = seed % CH
                    n = int(r["count"].view(-1)[b].item())
                    g = lambda k: (r[k] if r["count"].numel() > 1 else r[k].unsqueeze(0))[b, :n].cpu().numpy()
                    return {"ids": g("ids"), "LAFs": g("LAFs"), "resp": g("responses"), "desc": g("descriptors")}
                return fetch
            kept = [(s, w) for s, w in kept if s < args.batch]
            if kept:
                gb = args.batch if (H, W, NKP) == (768, 1024, 2000) else 0       # the golden vectors exist at the metric's configuration only
                out["parity_check"] = parity_check(kept, fetcher(last), golden_batch=gb)
                for mode, res_m in last_split.items():
                    if "value" in out.get("arith_" + mode, {}):
                        out["arith_" + mode]["parity_check"] = parity_check(kept, fetcher(res_m), tag=mode, golden_batch=gb)
                for _, w in kept:                                    # the extractor holds the image's pyramid, the referee its float64 copies
                    w.pop("ex", None); w.pop("ref", None)
        wall["total_since_process_start_s"] = round(time.time() - T_START, 1)
        out["wall_s"] = wall
        final = out
    else:
        final = None
    if DIST:
        dist.destroy_process_group()
    if final is not None:
        emit(final)                    # LAST: after the process group is gone (RCCL writes a version banner to the C stdout, flushed at exit)


def other_configs(nets, dev, arith, gpu_sections, with_cpu=True):
    """Short samples of the two other single-GPU BASELINE configurations, attached to the default line:
    configs[1] = single-image latency on graf img1 (eager + one HIP graph), configs[4] = 3840x2160 / 8000 kp (8 images per launch:
    1 warm-up + 2 timed steps, stage events, trunk roofline, tracked counter traffic) with a one-image CPU oracle baseline."""
    import numpy as np
    from PIL import Image
    import affnet_amd
    from affnet_amd import _lib
    from affnet_amd.synthetic import synthetic_image
    A, O, Hn = nets
    out = {}
    # ---- configs[1]
    img = np.mean(np.array(Image.open(GRAF).convert("RGB")), axis=2).astype(np.float32)
    host = torch.from_numpy(img).view(1, 1, img.shape[0], img.shape[1]).pin_memory()
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=2000, border=5, num_Baum_iters=1, AffNet=A, OriNet=O, arith=arith).to(dev)
    w0 = time.time()
    c2 = config2_measure(det, Hn, host, dev, 20, arith)
    gpu_sections.append({"what": "other_configs: configs[1] latency sample", "unix_start_s": w0, "unix_end_s": time.time()})
    out["config2_eager_ms"] = c2["value"]
    out["config2_graph_ms"] = c2["hip_graph"].get("warm_ms")
    out["config2_graph_identical_to_eager"] = c2["hip_graph"].get("identical_to_eager")
    out["config2_keypoints"] = c2["config"]["keypoints"]
    out["config2_workload"] = c2["config"]["workload"]
    del det
    # ---- configs[4]
    h5, w5, n5, b5 = 2160, 3840, 8000, 8
    x = torch.cat([synthetic_image(h5, w5, s) for s in range(b5)], 0).to(dev)
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=n5, border=5, num_Baum_iters=1, AffNet=A, OriNet=O, arith=arith).to(dev)
    ctx = det._context(x, allow_batch=True)
    r = det.enqueue(x, do_ori=True, desc=Hn)
    torch.cuda.synchronize()
    _lib.check(_lib.lib.affnet_profile_enable(ctx.handle, 1), ctx.handle, "profile_enable")
    steps5 = 3
    w0 = time.time()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps5 + 1)]
    evs[0].record()
    for i in range(steps5):
        r = det.enqueue(x, do_ori=True, desc=Hn)
        evs[i + 1].record()
    torch.cuda.synchronize()
    # median step (three back-to-back steps, HIP events between them): a one-off stall in a 2-step sample once showed up as 14 % (round 6 evidence run)
    per_step = sorted(evs[i].elapsed_time(evs[i + 1]) * 1e-3 for i in range(steps5))
    dt = per_step[steps5 // 2] * steps5
    gpu_sections.append({"what": "other_configs: configs[4] sample (%d steps of %d 4K images)" % (steps5, b5), "unix_start_s": w0, "unix_end_s": time.time()})
    ctx.read_counts(allow_empty=True)
    kp = int(r["count"].sum().item())
    buf, n = (C.c_double * 8)(), C.c_int32(0)
    _lib.check(_lib.lib.affnet_profile_read(ctx.handle, C.byref(buf), C.byref(n)), ctx.handle, "profile_read")
    _lib.check(_lib.lib.affnet_profile_enable(ctx.handle, 0), ctx.handle, "profile_enable")
    names = ["pyramid", "detector", "affnet", "shape_filter", "orinet", "denorm_levelsel", "hardnet_trunk", "hardnet_head"]
    stage = [v / max(n.value * b5, 1) for v in list(buf)]
    trunk_ms = list(buf)[6] / max(n.value, 1)
    fl = kp * (FLOP_HARD - FLOP_HARD_HEAD)
    tf = fl / (trunk_ms * 1e-3) / 1e12 if trunk_ms > 0 else 0.0
    traffic = config5_traffic()
    split3 = arith in SPLIT
    peak = PEAK_BF16_MFMA_TFLOPS if split3 else PEAK_FP32_MFMA_TFLOPS
    ach = SPLIT[arith]["products"] * (fl - kp * 2.0 * 1024 * 9 * 32) / (trunk_ms * 1e-3) / 1e12 if (split3 and trunk_ms > 0) else tf
    out["config5_kp_s"] = kp * steps5 / dt
    out["config5_ms_per_image"] = dt / (steps5 * b5) * 1e3
    out["config5_stage_ms"] = dict(zip(names, [round(v, 4) for v in stage]))
    out["config5_workload"] = "BASELINE.json configs[4]: %d synthetic %dx%d images per launch, %d kp each, median of %d timed steps after 1 warm-up" % (b5, w5, h5, n5, steps5)
    out["config5_roofline"] = {"kernel": "cnn32_trunk_kernel<HardNet>" + (" split operands" if split3 else " (fp32 MFMA 16x16x4)"), "bound": "mfma", "achieved": ach,
                               "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "flops_per_launch": fl, "launch_ms": trunk_ms,
                               "traffic": traffic.get("trunk_hbm_bytes_per_launch") if traffic else None,
                               "traffic_source": traffic.get("source") if traffic else None,
                               "scale_space": traffic.get("scale_space") if traffic else None}
    # host-independent parity leg of configs[4]: image 0 of the batch against the unmodified reference's output (tests/golden/make_golden_config3.py 4k)
    gpath = os.path.join(ROOT, "tests", "golden", "synth_%dx%d_s0_n%d.npz" % (h5, w5, n5))
    if os.path.isfile(gpath):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from _rowmatch import match_rows
        g = np.load(gpath)
        n0 = int(r["count"].view(-1)[0].item())
        Lg, rg, Dg = r["LAFs"][0, :n0].cpu().numpy(), r["responses"][0, :n0].cpu().numpy(), r["descriptors"][0, :n0].cpu().numpy()
        gi, wi = match_rows(rg, Lg, g["resp"], g["LAFs"])
        eg = np.abs(Lg[gi] - g["LAFs"][wi]).reshape(len(gi), -1).max(axis=1)
        dg = np.abs(Dg[gi] - g["desc"][wi].astype(np.float32)).max(axis=1)
        out["config5_golden"] = {"rows": int(len(g["resp"])), "matched": int(len(gi)), "rows_outside_1e-3": int((eg >= 1e-3).sum()), "laf_max_px": float(eg.max()),
                                 "desc_max": float(dg.max()), "pass": bool(len(gi) >= 0.995 * len(g["resp"]) and (eg < 1e-3).mean() >= 0.999 and eg.max() < 1e-2 and (dg[eg < 1e-3] < 1e-3).all()),
                                 "bar": ">= 99.5 % of the reference's rows matched, >= 99.9 % of the matched LAF rows within 1e-3 px, none outside 1e-2 px, descriptors (golden stored as float16) within 1e-3"}
    del det, x, r
    torch.cuda.empty_cache()
    if with_cpu:
        out["config5_cpu_baseline"] = cpu_baseline_one(h5, w5, n5)
    return out


def config5_traffic():
    """Calibrated FETCH_SIZE / WRITE_SIZE of the 4K run from the newest tracked profiles/*_config5_traffic.json (tools/gpu_pmc_c5.sh +
    tools/pmc_traffic.py: separate --pmc passes; counters cannot be read from inside this process)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_config5_traffic.json")))
    if not files:
        return None
    d = json.load(open(files[-1]))
    ks = d.get("kernels", {})
    trunk = next((v for k, v in ks.items() if "cnn32_trunk_kernel<2, 8, false, false>" in k or "cnn32_trunk_kernel<2, 8, false, 0>" in k), None)
    ss = {k.split("(")[0].replace("void ", "")[:60]: {"hbm_bytes_per_launch": v.get("hbm_bytes"), "fetch_bytes": v.get("fetch_bytes"), "write_bytes": v.get("write_bytes")}
          for k, v in ks.items() if "blur2d" in k or "hessian_nms" in k}
    return {"trunk_hbm_bytes_per_launch": trunk.get("hbm_bytes") if trunk else None, "scale_space": ss,
            "source": "%s (%d images per launch; %s)" % (os.path.basename(files[-1]), d.get("images_per_launch", 0), d.get("correction", ""))}


def cpu_baseline_one(h, w, nkp, threads=16):
    """One image of another configuration through the CPU oracle on this host (no warm-up at this size): kp/s."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import affnet_oracle as orc
    sd = {k: torch.load(os.path.join(ROOT, "pretrained", k + ".pth"), map_location="cpu", weights_only=False)["state_dict"] for k in ("AffNet", "OriNet")}
    hard = orc.synthetic_hardnet_state(0)
    avail, phys = host_threads()
    t = max(1, min(threads, phys))
    prev = torch.get_num_threads()
    torch.set_num_threads(t)
    try:
        x = orc.synthetic_image(h, w, 0)
        ex = orc.OracleExtractor(mrSize=5.192, num_features=nkp, border=5, num_Baum_iters=1, affnet_sd=sd["AffNet"], orinet_sd=sd["OriNet"],
                                 reproduce_wasted_extraction=True)
        t0 = time.perf_counter()
        L, r, P, D = orc.describe(x, ex, hard, do_ori=True, ps=32)
        dt = time.perf_counter() - t0
    finally:
        torch.set_num_threads(prev)
    return {"value": L.shape[0] / dt, "unit": "keypoints/s", "cores": t, "kind": "port", "seconds": dt,
            "sample": "ONE synthetic %dx%d image x %d kp (seed 0), %d threads, no warm-up at this size" % (w, h, nkp, t)}


def verify_gather(records, mode, world, rank, batch, dev, nets, onepass):
    """The N-rank path checked with REAL kernels: rank 0 takes the records the exchange delivered for the last timed step (global
    image order: image i was computed by rank i % world from seed i) and re-computes the checked ones itself with a single-image call on
    the same seed: equal count, bit-equal LAFs / responses / descriptors (batched == single-image is bit-exact, tests/test_gpu_parity.py).
    Wrong order, a swapped rank, stale or truncated records all show here.  Returns the dict for the bench line (rank 0) or None."""
    import affnet_amd
    from affnet_amd import sharded
    from affnet_amd.synthetic import synthetic_image
    if rank != 0:
        return None
    n_total = batch * world
    if records is None or records.size(0) != n_total:
        return {"identical": False, "error": "rank 0 holds %s records, expected %d" % (None if records is None else records.size(0), n_total)}
    if mode == "all":
        idx = list(range(n_total))
    else:                                         # first and last image of every rank
        idx = sorted(set([r for r in range(world)] + [r + world * (batch - 1) for r in range(world)]))
    A, O, Hn = nets
    if onepass:
        return {"identical": None, "error": "not implemented for --onepass"}
    det = affnet_amd.ScaleSpaceAffinePatchExtractor(mrSize=5.192, num_features=NKP, border=5, num_Baum_iters=1, AffNet=A, OriNet=O).to(dev)
    bad, counts = [], sharded.record_counts(records).tolist()
    for i in idx:
        res = det.run(synthetic_image(H, W, i).to(dev), do_ori=True, desc=Hn)
        got = sharded.unpack_record(records[i], NKP)
        n = int(res["LAFs"].shape[0])
        same = counts[i] == n and all(torch.equal(got[k], res[k]) for k in ("LAFs", "responses", "descriptors"))
        if not same:
            bad.append({"record": i, "from_rank": i % world, "count_gathered": counts[i], "count_recomputed": n})
    return {"records": n_total, "checked": len(idx), "mode": mode, "identical": not bad, "mismatches": bad[:8],
            "what": "gathered record i of the last timed step vs a single-image call on seed i by rank 0: count, LAFs, responses, "
                    "descriptors bit-equal, global order i -> rank i % world"}


def secondary_rooflines(dets, chunks, stage_ms, dev):
    """north_star: HBM GB/s of the scale-space / grid-sample kernels against chip peak.  Algorithmic bytes (SURVEY.md section
    8d) / HIP-event time: pyramid and detector from the stage events of the timed region, the sampler from a stand-alone run
    of affnet_pyr_grid_sample over 7000 patches per image (3000 detector candidates + 2 x 2000 level-selected final frames)."""
    import numpy as np
    from affnet_amd import _lib, engine
    from affnet_amd._lib import lib, ptr, check
    det = next(iter(dets.values()))
    ctx = det._ctx
    plan = ctx.plan
    P0 = H * W
    P = sum(h * w for h, w in plan.sizes)
    L = plan.levels_per_octave
    out = []
    pyr_bytes = (P0 + (L - 1) * P + L * P) * 4.0            # read the image + L-1 levels, write L levels (decimated copies are part of P)
    det_bytes = L * P * 4.0                                  # every level read once; responses never reach HBM
    # pyramid: bound by the fp32 VECTOR rate (the bit-exact 2-D tap order is k x k fused multiply-adds per pixel: ~6x the MACs of a
    # separable blur, 1.4 GFLOP per image against 41 MB of traffic); the HBM rate north_star asks for stays as a secondary field
    from affnet_amd.host_plan import gaussian_taps
    ksq = lambda sg: float(gaussian_taps(sg).shape[0]) ** 2
    flops = (ksq(plan.first_blur_sigma) * P0 if plan.first_blur_sigma else 0.0)
    for o, (h_o, w_o) in enumerate(plan.sizes):
        flops += sum(ksq(sg) for sg in plan.blur_sigmas_per_octave[o]) * h_o * w_o      # levels 1 .. L-1
    flops *= 2.0
    ms = stage_ms[0]
    tf = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    gbs = pyr_bytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    out.append({"kernel": "blur2d_kernel<K> / blur2d_pair_kernel (pyramid build: %d launches per call, exact 2-D taps)" % (1 + (L - 2) * plan.n_octaves + 1),
                "bound": "valu", "algorithmic_flops_per_image": flops, "ms_per_image": ms, "achieved": tf, "peak": PEAK_FP32_MFMA_TFLOPS,
                "unit": "TFLOP/s", "frac": tf / PEAK_FP32_MFMA_TFLOPS,
                "hbm": {"algorithmic_bytes_per_image": pyr_bytes, "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS},
                "note": "fp32 vector peak = the fp32 matrix peak (157.3 TFLOP/s, MI355X_MICROARCH.md); VALU-bound by design: the bit-exact k x k tap "
                        "order costs ~6x the MACs of a separable blur"})
    ms = stage_ms[1]
    gbs = det_bytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    out.append({"kernel": "hessian_nms_kernel (+ level_resolve / select kernels = detector stage)", "bound": "hbm", "algorithmic_bytes_per_image": det_bytes,
                "ms_per_image": ms, "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS,
                "note": "Hessian + 3-D NMS + centroid fused, responses stay on chip; latency / LDS bound, not bandwidth bound (DESIGN.md section 4)"})
    # stand-alone sampler on the pyramids of the chunk processed last
    x = chunks[0]
    if x.size(0) != ctx.batch:
        return out
    B, Pc, F = ctx.batch, ctx.cap_pre, ctx.cap_final
    st = engine.stream_of(dev)
    r = det.enqueue(x, do_ori=True, desc=None)              # leaves pyramid + final LAFs
    lafs_px = (r["LAFs"] if B > 1 else r["LAFs"].unsqueeze(0)).contiguous()
    cnt = r["count"]
    d_resp = torch.empty(B, Pc, dtype=torch.float32, device=dev)
    d_lafs = torch.empty(B, Pc, 2, 3, dtype=torch.float32, device=dev)
    d_ids = torch.empty(B, Pc, 3, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    check(lib.affnet_detect(ctx.handle, ptr(d_resp), ptr(d_lafs), ptr(d_ids), ptr(d_cnt), st), ctx.handle, "affnet_detect")
    f_ids = torch.empty(B, F, 3, dtype=torch.int32, device=dev)
    f_norm = torch.empty(B, F, 2, 3, dtype=torch.float32, device=dev)
    check(lib.affnet_level_select(ctx.handle, ptr(lafs_px), ptr(cnt), F, 32, ptr(f_ids), ptr(f_norm), st), ctx.handle, "affnet_level_select")
    out_c = torch.empty(B, Pc, 32, 32, dtype=torch.float32, device=dev)
    out_f = torch.empty(B, F, 32, 32, dtype=torch.float32, device=dev)

    def sample_all():
        check(lib.affnet_pyr_grid_sample(ctx.handle, ptr(d_lafs), ptr(d_ids), ptr(d_cnt), Pc, 32, ptr(out_c), st), ctx.handle, "grid_sample")
        for _ in range(2):
            check(lib.affnet_pyr_grid_sample(ctx.handle, ptr(f_norm), ptr(f_ids), ptr(cnt), F, 32, ptr(out_f), st), ctx.handle, "grid_sample")
    for _ in range(2):
        sample_all()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 5
    e0.record()
    for _ in range(reps):
        sample_all()
    e1.record()
    torch.cuda.synchronize()
    ms_img = e0.elapsed_time(e1) / reps / B
    # algorithmic bytes: 4096 B written per patch + the source footprint (bounding box of the sampled frame in level pixels, + 1 px
    # for the bilinear neighbours) read once
    sizes = np.array(plan.sizes, dtype=np.float64)

    def footprint(lafs, ids, counts):
        lafs, ids, counts = lafs.cpu().numpy().astype(np.float64), ids.cpu().numpy(), counts.cpu().numpy()
        tot, n = 0.0, 0
        for b in range(lafs.shape[0]):
            k = int(counts[b])
            o = np.clip(ids[b, :k, 0], 0, len(sizes) - 1)
            h, w = sizes[o, 0], sizes[o, 1]
            m = np.minimum(h, w)
            A = lafs[b, :k, :, :2] * m[:, None, None] * (31.0 / 32.0)     # half extents in level px (grid = +-(ps-1)/ps)
            hx = np.abs(A[:, 0, 0]) + np.abs(A[:, 0, 1])
            hy = np.abs(A[:, 1, 0]) + np.abs(A[:, 1, 1])
            tot += float((np.minimum(2 * hx + 2, w) * np.minimum(2 * hy + 2, h)).sum()) * 4.0
            n += k
        return tot, n
    fc, nc = footprint(d_lafs, d_ids, d_cnt)
    ff, nf = footprint(f_norm, f_ids, cnt)
    patches = nc + 2 * nf
    # HBM-relevant algorithmic bytes: every patch is written once (4096 B); the source pixels are shared by overlapping patches,
    # so what must come from HBM is at most the pyramid levels that are touched at all (the per-patch footprints add up to several
    # times that and are served by L2 / Infinity Cache)
    def touched(ids, counts):
        ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
        tot = 0.0
        for b in range(ids.shape[0]):
            k = int(counts[b])
            lv = {(int(o), int(l)) for o, l in zip(ids[b, :k, 0], ids[b, :k, 1])}
            tot += sum(sizes[min(max(o, 0), len(sizes) - 1)].prod() * 4.0 for o, l in lv)
        return tot
    src = min(fc, touched(d_ids, d_cnt)) + 2 * min(ff, touched(f_ids, cnt))
    bts = (src + 4096.0 * patches) / B
    foot = (fc + 2 * ff + 4096.0 * patches) / B
    gbs = bts / (ms_img * 1e-3) / 1e9
    out.append({"kernel": "grid_sample_kernel stand-alone (affnet_pyr_grid_sample, PS 32, %.0f patches per image = C + 2N)" % (patches / B), "bound": "hbm",
                "algorithmic_bytes_per_image": bts, "bytes_per_patch": bts * B / max(patches, 1), "ms_per_image": ms_img, "achieved": gbs,
                "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS,
                "footprint_sum_bytes_per_image": foot, "footprint_rate_GBs_incl_cache_hits": foot / (ms_img * 1e-3) / 1e9,
                "survey_8KB_per_patch_rate_GBs": 8192.0 * patches / B / (ms_img * 1e-3) / 1e9,
                "note": "algorithmic bytes = 4096 B written per patch + the pyramid levels the patches touch, read once (overlapping "
                        "footprints - %.1f KB per patch on these LAFs - are cache hits); in the product path the sampler is fused into the "
                        "CNN trunk prologues (no patch tensor in HBM), this is the stand-alone kernel the foreign-slot path and "
                        "extract_patches_from_pyr use" % ((fc + 2 * ff) / max(patches, 1) / 1024.0)})
    return out


def dry_run(args, world, rank, dist, sharded, DIST, gather_dst, backend):
    """CPU bookkeeping run of the multi-rank path: rendezvous, world-size / device checks, round-robin seeds, record
    packing and the gather, one JSON line from rank 0.  No kernels, no timing claims."""
    n_cap = 5
    got = None
    for step in range(max(1, args.steps)):
        seeds = [rank + world * j for j in range(args.batch)]
        res = []
        for s in seeds:
            g = torch.Generator().manual_seed(1000 * step + s)
            n = 1 + s % n_cap
            r = {"count": torch.tensor([n], dtype=torch.int32), "LAFs": torch.zeros(n_cap, 2, 3), "responses": torch.zeros(n_cap),
                 "descriptors": torch.zeros(n_cap, 128)}
            r["LAFs"][:n] = torch.rand(n, 2, 3, generator=g)
            r["responses"][:n] = float(s)
            res.append(r)
        rec = sharded.pack_records(res, n_cap, torch.device("cpu"))
        got = sharded.gather_features_async(rec, args.batch * world, dst=gather_dst)() if DIST else rec
    ok = True
    if got is not None:
        cnt = sharded.record_counts(got).tolist()
        ok = cnt == [1 + i % n_cap for i in range(args.batch * world)]
        ok &= all(float(sharded.unpack_record(got[i], n_cap)["responses"][0]) == float(i) for i in range(args.batch * world))
    flag = torch.tensor([1.0 if ok else 0.0])
    if DIST:
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if DIST:
        dist.destroy_process_group()
    if rank == 0:
        emit({"dry_run": True, "metric": "keypoints/sec (detect+AffNet+OriNet+HardNet) per image, %d kp @%dx%d" % (NKP, W, H),
              "value": None, "unit": "keypoints/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True,
              "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic (dry run: fake records, no kernels)",
              "config": {"workload": "dry run of the N-rank bookkeeping", "global_batch": args.batch * world, "images_per_launch": args.chunk,
                         "parallelism": "image-per-GPU x%d, %s over %s" % (world, "all_gather" if gather_dst is None else "gather to rank 0", backend)},
              "exchange": {"mode": "all_gather" if gather_dst is None else "gather_rank0", "exchange_bytes_per_step": int(got.numel()) * 4 * (world if gather_dst is None else 1)
                           if got is not None else None, "gather_ms": None},
              "ms_per_step_per_rank": {"min": None, "max": None},
              "records_in_global_order": bool(flag.item() == 1.0)})
    if flag.item() != 1.0:
        sys.exit(3)


if __name__ == "__main__":
    main()
