#!/usr/bin/env python
"""Per-phase cycle breakdown of the fused CNN trunk kernels (s_memtime stamps, tuning aid).
Runs each net on 2048 random patches and prints mean cycles per phase per wave."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import affnet_amd
from affnet_amd._lib import lib, ptr
from affnet_amd import engine

dev = torch.device("cuda:0")
n = int(os.environ.get("PHASE_PATCHES", "2048"))      # 256 = one workgroup per CU: the phases without a co-resident workgroup
p = (torch.rand(n, 1, 32, 32) * 255).to(dev)
A = affnet_amd.AffNetFast(); A.load_state_dict(torch.load(os.path.join(ROOT, "pretrained/AffNet.pth"), map_location="cpu", weights_only=False)["state_dict"]); A.to(dev)
O = affnet_amd.OriNetFast(); O.load_state_dict(torch.load(os.path.join(ROOT, "pretrained/OriNet.pth"), map_location="cpu", weights_only=False)["state_dict"]); O.to(dev)
H = affnet_amd.HardNet(); H.load_state_dict(affnet_amd.synthetic_hardnet_state(0)); H.to(dev)
names = ["input+norm", "conv0", "conv1 mfma", "conv1 store", "conv2 mfma", "conv2 store", "conv3 mfma", "conv3 store",
         "conv4 mfma", "conv4 store", "conv5 mfma", "conv5 store"]
only = os.environ.get("PHASE_NETS")                    # e.g. PHASE_NETS=OriNet: that net's table alone


class AffNetForm1:
    """AffNet's Winograd trunk (conv1 / conv3 / conv5 as F(2x2, 3x3)), which the fused shape pass runs on every candidate in shape form 1: the trunk launch alone
    (head partials, no finish kernel) through the probe library (AFFNET_HIP_LIB=affnet_amd/libaffnet_hip_probes.so).  probe = affnet_probe_affnet_poly_partials: the
    trunk of shape form 2 instead (conv2 / conv4 as polyphase Winograd F(2x2, 2x2) besides)"""
    def __init__(self, probe="affnet_probe_affnet_wino_partials"):
        self.probe = getattr(lib, probe)

    def __call__(self, x):
        part = torch.empty(x.shape[0] * 32, device=dev)
        packed = A.packed_weights(dev)
        for i in range(0, x.shape[0], 65535):
            m = min(65535, x.shape[0] - i)
            rc = self.probe(engine.utility_ctx(dev), ptr(packed), ptr(x[i:i + m]), m, ptr(part[i * 32:]), None)
            assert rc == 0, rc
        return part


class HardNetForm1:
    """HardNet's trunk of descriptor form 1 (conv2 / conv4 as polyphase Winograd F(2x2, 2x2)) or 2 (conv3 as F(4x4, 3x3) besides), which the fused calls run and
    HardNet.forward never does: trunk + head on a patch tensor through the probe library (AFFNET_HIP_LIB=affnet_amd/libaffnet_hip_probes.so)"""
    def __init__(self, probe="affnet_probe_hardnet_poly_forward"):
        self.probe = getattr(lib, probe)

    def __call__(self, x):
        out = torch.empty(x.shape[0], 128, device=dev)
        packed = H.packed_weights(dev)
        rows = min(x.shape[0], 16384)
        scratch = torch.empty(rows * (8192 + 512), device=dev)
        for i in range(0, x.shape[0], rows):
            m = min(rows, x.shape[0] - i)
            rc = self.probe(engine.utility_ctx(dev), ptr(packed), ptr(x[i:i + m]), m, ptr(out[i:i + m]), ptr(scratch), None)
            assert rc == 0, rc
        return out


nets = [(A, "AffNet", 8), (O, "OriNet", 8), (H, "HardNet", 8)]
if hasattr(lib, "affnet_probe_hardnet_poly_forward"):
    nets.append((HardNetForm1(), "HardNet form 1", 8))
    if hasattr(lib, "affnet_probe_hardnet_f43_forward"):
        nets.append((HardNetForm1("affnet_probe_hardnet_f43_forward"), "HardNet form 2", 8))
    if hasattr(lib, "affnet_probe_hardnet_c5_forward"):
        nets.append((HardNetForm1("affnet_probe_hardnet_c5_forward"), "HardNet form 3", 8))
    if hasattr(lib, "affnet_probe_hardnet_c1_forward"):
        nets.append((HardNetForm1("affnet_probe_hardnet_c1_forward"), "HardNet form 4", 8))
else:
    print("(no table of HardNet's polyphase trunk: this library has no affnet_probe_hardnet_poly_forward - AFFNET_HIP_LIB=affnet_amd/libaffnet_hip_probes.so)")
if hasattr(lib, "affnet_probe_affnet_wino_partials"):
    nets.insert(1, (AffNetForm1(), "AffNet form 1", 8))
    if hasattr(lib, "affnet_probe_affnet_poly_partials"):
        nets.insert(2, (AffNetForm1("affnet_probe_affnet_poly_partials"), "AffNet form 2", 8))
else:
    print("(no table of AffNet's Winograd trunk: this library has no affnet_probe_affnet_wino_partials - AFFNET_HIP_LIB=affnet_amd/libaffnet_hip_probes.so)")
wg_ticks = {}                                          # per table: mean ticks of a workgroup from its first stamp 0 to its last stamp 13 (start to end of the trunk kernel)
for net, nm, nw in nets:
    if only and nm not in only.split(","):
        continue
    net(p); torch.cuda.synchronize()
    st = torch.zeros(n * nw * 32, dtype=torch.int64, device=dev)
    lib.affnet_cnn32_debug_timing(engine.utility_ctx(dev), ptr(st))
    net(p); torch.cuda.synchronize()
    lib.affnet_cnn32_debug_timing(engine.utility_ctx(dev), None)
    t = st.cpu().numpy().reshape(n, nw, 32).astype(np.float64)
    cut5 = nm in ("HardNet form 3", "HardNet form 4")
    nms = names
    nst = 10 if cut5 else 12                        # the trunk of forms 3 / 4 ends behind conv4's loop (stamps 0 .. 9, then 13); conv5 is a kernel of its own, tabled below
    if nm == "HardNet form 4":                      # conv0 + conv1 streamed: stamp 2 stands behind the first quarter's loop, stamp 3 behind the last quarter's
        nms = ["input+norm", "c0 half+q0", "c0 half+q1-3", "conv1 out+st"] + names[4:]
    d = np.diff(t[:, :, :nst], axis=2)              # cycles per phase per wave
    wg = t[:, :, :nst].max(axis=1) - t[:, :, 0:1].min(axis=1)   # per patch: boundary times relative to WG start
    print("== %s (%d waves): mean phase cycles per wave (s_memtime ticks, 100 MHz const clock?)" % (nm, nw))
    tot = (t[:, :, nst - 1].max(axis=1) - t[:, :, 0].min(axis=1)).mean()
    span = (t[:, :, nst - 1].max() - t[:, :, 0].min())
    print("  kernel span %.0f ticks for %d patches -> %.0f ticks / patch / CU-slot (256 CUs)" % (span, n, span / (n / 256.0)))
    for i in range(nst - 1):
        print("  %-12s mean %9.0f  max-over-waves %9.0f" % (nms[i], d[:, :, i].mean(), d[:, :, i].max(axis=1).mean()))
    print("  total per patch (WG) %.0f ticks" % tot)
    simd = (st.cpu().numpy().reshape(n, nw, 32)[:, :, 14] >> 4) & 3
    for i in (j for j in (2, 6, 10) if j < nst - 1):
        print("  %-12s per wave:" % nms[i], " ".join("%6.0f" % v for v in d[:, :, i].mean(axis=0)))
    # the two waves of a workgroup that share a SIMD: how far apart do they finish a loop?
    first, second = [], []
    for k in range(0, n, max(1, n // 128)):
        for sd in range(4):
            w = np.where(simd[k] == sd)[0]
            if len(w) == 2:
                a, b = d[k, w[0], 2], d[k, w[1], 2]
                first.append(min(a, b)); second.append(max(a, b))
    if first:
        print("  conv1 mfma, SIMD-sharing pairs: faster wave %.0f, slower wave %.0f ticks; SIMD ids of waves 0..%d in patch 0: %s" %
              (np.mean(first), np.mean(second), nw - 1, simd[0].tolist()))
    ti = st.cpu().numpy().reshape(n, nw, 32)
    start, end = ti[:, :, 0].min(axis=1).astype(np.float64), ti[:, :, 13].max(axis=1).astype(np.float64)
    wg_ticks[nm] = float((end - start).mean())
    print("  workgroup, first stamp 0 -> last stamp 13: %.0f ticks" % wg_ticks[nm])
    print("  last phase stamp -> kernel end (head / global store): %.0f ticks" % (ti[:, :, 13] - ti[:, :, nst - 1]).mean())
    hw, xcc = ti[:, 0, 14], ti[:, 0, 15] & 0xF
    cu = ((hw >> 8) & 0xF) | (((hw >> 12) & 1) << 4) | (((hw >> 13) & 7) << 5) | (xcc << 8)
    util, gaps = [], []
    for c in np.unique(cu):
        idx = np.where(cu == c)[0]
        s_, e_ = start[idx], end[idx]
        o = np.argsort(s_)
        s_, e_ = s_[o], e_[o]
        span = e_.max() - s_.min()
        util.append((e_ - s_).sum() / span)
        # gap between a WG ending and the next WG starting on this CU (slot-agnostic: sorted ends vs later starts)
        ends = np.sort(e_)
        for k in range(len(s_)):
            prev = ends[ends <= s_[k]]
            if len(prev):
                gaps.append(s_[k] - prev.max())
    sub = t[:, :, [0, 16, 17, 18, 1, 19, 20, 2]]
    ds = np.diff(sub, axis=2).mean(axis=(0, 1))
    if nm == "HardNet form 4":
        # the slots of the phases this form does not have: 19 conv0 of K group 0 + barrier | 20 first quarter's transform + barrier | 2 its loop | 3 last quarter's loop |
        # 21 output transform + barrier | 22 halo + stores | 4 barrier.  Mean over waves [max over waves]; the model's line (NOTES.md) beside each
        dm = np.diff(sub, axis=2).max(axis=1).mean(axis=0)
        print("  input: load %.0f | halo+sum1 %.0f | sum2 %.0f | patch write+barrier %.0f" % tuple(ds[:4]))
        print("  conv0 + conv1 streamed:            mean [max over waves]   model")
        print("    conv0 half + barrier             %6.0f [%6.0f]          3.4 k" % (ds[4], dm[4]))
        print("    quarter transform + barrier      %6.0f [%6.0f]          2.7 k" % (ds[5], dm[5]))
        print("    quarter loop (72 MFMAs)          %6.0f [%6.0f]          4.9 k" % (ds[6], dm[6]))
        rest = np.diff(t[:, :, [2, 3]], axis=2)
        print("    second half + quarters 1 - 3     %6.0f [%6.0f]          3.4 k + 3 x 7.6 k = 26.2 k" % (rest.mean(), rest.max(axis=1).mean()))
        ep = np.diff(t[:, :, [3, 21, 22, 4]], axis=2)
        print("    output transform + barrier %.0f | halo + stores %.0f | barrier %.0f [sum of max over waves %.0f]   about 7 k" %
              (tuple(ep.mean(axis=(0, 1))) + (ep.max(axis=1).mean(axis=0).sum(),)))
        c1 = (t[:, :, 4].max(axis=1) - t[:, :, 1].min(axis=1)).mean()
        print("    conv0 + conv1, first stamp 1 -> last stamp 4: %.0f ticks (model about 44 k; form 3: conv0 6.3 k + conv1 loop 42.8 k + store 7.9 k, critical path about 52.5 k)" % c1)
    else:
        print("  input: load %.0f | halo+sum1 %.0f | sum2 %.0f | patch write+barrier %.0f || conv0: mfma %.0f | stores %.0f | barrier %.0f" % tuple(ds))
        sub = t[:, :, [3, 21, 22, 4]]
        ds = np.diff(sub, axis=2).mean(axis=(0, 1))
        print("  conv1 epilogue: barrier1 %.0f | halo+stores %.0f | barrier2 %.0f" % tuple(ds))
        c1 = (t[:, :, 4].max(axis=1) - t[:, :, 1].min(axis=1)).mean()
        print("  conv0 + conv1, first stamp 1 -> last stamp 4: %.0f ticks" % c1)
    if nm in ("HardNet form 2", "HardNet form 3", "HardNet form 4"):        # "conv3 mfma" = stamp 6 -> 7 spans the whole F(4x4, 3x3) layer but its store
        ds = np.diff(t[:, :, [6, 23, 7]], axis=2).mean(axis=(0, 1))
        print("  conv3 F(4x4, 3x3): transform + V through LDS + loop + fold along x %.0f | barrier + exchange of the halves %.0f" % tuple(ds))
    if cut5:
        # hardnet_conv5_f43_kernel, one workgroup per four patches: stamps 24 .. 31 of every wave in the record of the group's first patch
        # 24 start | 25 quarter 0 in LDS | 26 its transform done | 27 its loop done | 28 quarter 3's transform done | 29 its loop done | 30 output transform done | 31 stored
        g = t[0::4, :, 24:32]
        dg = np.diff(g, axis=2)
        c5 = (g[:, :, 7].max(axis=1) - g[:, :, 0].min(axis=1)).mean()
        print("  conv5 kernel (%d groups of four patches): mean ticks per wave [max over waves]" % g.shape[0])
        for i, what in enumerate(("input of quarter 0: load + LDS + barrier", "transform of quarter 0 (+ barrier)", "loop of quarter 0 (288 MFMAs)", "quarters 1, 2 and 3 up to its transform",
                                  "loop of quarter 3 (288 MFMAs)", "barrier + output transform", "bias, ReLU, store")):
            print("    %-42s %9.0f [%9.0f]" % (what, dg[:, :, i].mean(), dg[:, :, i].max(axis=1).mean()))
        print("    loop of quarter 0: %.1f cycles per MFMA" % (dg[:, :, 2].max(axis=1).mean() / 288.0))
        print("    workgroup, first stamp 24 -> last stamp 31: %.0f ticks = %.0f per patch" % (c5, c5 / 4.0))
        wg_ticks[nm + " + conv5"] = wg_ticks[nm] + c5 / 4.0
        if nm == "HardNet form 4" and "HardNet form 3 + conv5" in wg_ticks:
            f3, f4 = wg_ticks["HardNet form 3 + conv5"], wg_ticks[nm + " + conv5"]
            print("  GATE: form 4 trunk %.0f + conv5 kernel per patch %.0f = %.0f ticks against form 3's %.0f: %.0f ticks shorter (needed: 4000 or more)" % (wg_ticks[nm], c5 / 4.0, f4, f3, f3 - f4))
        if nm == "HardNet form 3" and "HardNet form 2" in wg_ticks:
            f3 = wg_ticks[nm] + c5 / 4.0
            print("  GATE: form 3 trunk %.0f + conv5 kernel per patch %.0f = %.0f ticks against form 2's workgroup %.0f: %.1f %% shorter (needed: 5 %% or more)" %
                  (wg_ticks[nm], c5 / 4.0, f3, wg_ticks["HardNet form 2"], 100.0 * (1.0 - f3 / wg_ticks["HardNet form 2"])))
    if nm in ("AffNet form 2", "OriNet") and t[:, :, 24].min() > 0:        # polyphase conv4: "conv4 mfma" = stamp 8 -> 9 spans the loop and the pair's exchange
        ds = np.diff(t[:, :, [8, 24, 9]], axis=2).mean(axis=(0, 1))
        print("  conv4 polyphase: loop %.0f | exchange of the K groups' partial y (one barrier) %.0f" % tuple(ds))
    print("  CUs seen %d; mean resident WGs per CU %.2f; median end->next-start gap %.0f ticks (p90 %.0f)" %
          (len(util), np.mean(util), np.median(gaps), np.percentile(gaps, 90)))
    # wall time of the same launch without stamps
    lib.affnet_cnn32_debug_timing(engine.utility_ctx(dev), None)
    big = (torch.rand(48000, 1, 32, 32) * 255).to(dev)
    net(big); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); net(big); e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    fl = {"AffNet": 19193856.0, "AffNet form 1": 19193856.0, "AffNet form 2": 19193856.0, "OriNet": 19316736.0, "HardNet": 78184448.0, "HardNet form 1": 78184448.0, "HardNet form 2": 78184448.0, "HardNet form 3": 78184448.0, "HardNet form 4": 78184448.0}[nm]      # direct-form FLOP per patch
    print("  48000 contiguous patches: %.3f ms -> %.1f TFLOP/s (incl. head / allocation)" % (ms, 48000 * fl / ms / 1e9))
