#!/usr/bin/env python
"""Register / LDS / scratch budget of every device kernel in the built objects (affnet_amd/csrc/obj/*.o), read from the code
objects' own metadata - what the hardware is told, not what a comment says.

    python tools/kernel_resources.py                 -> markdown table (profiles/r04_kernel_resources.md is this output)
    python tools/kernel_resources.py --json          -> {kernel: {...}}

The metadata notes list a kernel's fields alphabetically: `.group_segment_fixed_size` stands BEFORE `.name` and belongs to the
kernel named after it, `.private_segment_fixed_size` / `.vgpr_count` / `.vgpr_spill_count` stand after `.name` (reading the
LDS size off the lines that follow a name gives the NEXT kernel's value).  This parser keeps the fields of one `- .agpr_count`
... block together.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size", "max_flat_workgroup_size")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def demangle(names):
    if not names:                 # (with no operands the demanglers would wait on stdin)
        return []
    for tool in ("/usr/bin/c++filt", os.path.join(LLVM, "llvm-cxxfilt")):
        try:
            out = subprocess.run([tool] + list(names), capture_output=True, text=True, check=True, stdin=subprocess.DEVNULL,
                                 timeout=60).stdout.strip().split("\n")
            if len(out) == len(names):
                return out
        except Exception:
            pass
    return list(names)


def object_kernels(obj):
    """[{name, field: value, ...}] of one host object with an embedded gfx950 code object."""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
        # explicit output file: without one llvm-objcopy rewrites its INPUT in place (same bytes, new mtime - and build.sh compares mtimes)
        r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(td, "copy.o")], capture_output=True)
        if r.returncode != 0 or not os.path.isfile(fat):      # a translation unit without device code (host glue only)
            return []
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat,
                        "--output=" + co], check=True, capture_output=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = [], None
    in_kernels = False
    for line in notes.splitlines():
        if line.strip().startswith("amdhsa.kernels:"):
            in_kernels = True
            continue
        if not in_kernels:
            continue
        if re.match(r"^\s*amdhsa\.", line):          # next top-level key (amdhsa.target, amdhsa.version)
            break
        m = re.match(r"^(\s*)- \.(\w+):\s*(.*)$", line)
        if m and len(m.group(1)) <= 2:                # a new kernel block ("  - .agpr_count: 0")
            cur = {}
            kernels.append(cur)
            key, val = m.group(2), m.group(3)
        else:
            m = re.match(r"^\s+\.(\w+):\s*(.*)$", line)
            if not m or cur is None:
                continue
            key, val = m.group(1), m.group(2)
        if key == "name":
            cur["name"] = val.strip()
        elif key in FIELDS:
            cur[key] = int(val)
    return [k for k in kernels if "name" in k]


def all_kernels(obj_dir=None):
    obj_dir = obj_dir or os.path.join(ROOT, "affnet_amd", "csrc", "obj")
    out = {}
    for f in sorted(os.listdir(obj_dir)):
        if not f.endswith(".o"):
            continue
        ks = object_kernels(os.path.join(obj_dir, f))
        for k, dn in zip(ks, demangle([k["name"] for k in ks])):
            k["object"] = f
            k["demangled"] = re.sub(r"\(.*\)$", "", dn.replace("void ", "", 1))
            out[k["name"]] = k
    return out


def workgroups_per_cu(k):
    """Resident workgroups per CU by LDS (160 KB) and by registers (512 VGPRs per SIMD lane, waves of the workgroup spread over 4 SIMDs)."""
    lds = k.get("group_segment_fixed_size", 0)
    by_lds = 32 if lds == 0 else (160 * 1024) // lds
    waves = max(1, k.get("max_flat_workgroup_size", 256) // 64)
    regs = max(1, k.get("vgpr_count", 0) + k.get("agpr_count", 0))
    regs = (regs + 7) // 8 * 8
    waves_per_simd = min(8, 512 // regs)
    by_regs = (waves_per_simd * 4) // waves
    return max(0, min(by_lds, by_regs, 32))


# the kernels DESIGN.md section 4 quotes figures for (substring of the demangled name -> label)
DESIGN_KERNELS = [
    ("cnn32_trunk_kernel<2, 8, false, 0>", "HardNet trunk, exact fp32 MFMA"),
    ("cnn32_trunk_kernel<2, 8, false, 1>", "HardNet trunk, exact fp32 MFMA, polyphase Winograd conv2 / conv4 (descriptor form 1)"),
    ("cnn32_trunk_kernel<2, 8, false, 4>", "HardNet trunk, exact fp32 MFMA, form 1 with conv3 as Winograd F(4x4, 3x3) (descriptor form 2)"),
    ("cnn32_trunk_kernel<2, 8, false, 6>", "HardNet trunk, exact fp32 MFMA, form 2 cut behind conv4 (descriptor form 3)"),
    ("cnn32_trunk_kernel<2, 8, false, 7>", "HardNet trunk, exact fp32 MFMA, form 3 with conv0 + conv1 streamed, conv1 as Winograd F(4x4, 3x3) (descriptor form 4, default)"),
    ("hardnet_conv5_f43_kernel<false>", "HardNet conv5 as Winograd F(4x4, 3x3), four patches per workgroup (descriptor forms 3 / 4)"),
    ("cnn32_trunk_kernel<2, 8, false, 3>", "HardNet trunk, arith fp32_split3"),
    ("cnn32_trunk_kernel<2, 8, false, 2>", "HardNet trunk, arith fp32_split2h"),
    ("cnn32_trunk_kernel<0, 8, false, 0>", "AffNet trunk, exact fp32 MFMA"),
    ("cnn32_trunk_kernel<0, 8, false, 1>", "AffNet trunk, exact fp32 MFMA, Winograd conv1 / conv3 / conv5 (shape form 1)"),
    ("cnn32_trunk_kernel<0, 8, false, 5>", "AffNet trunk, exact fp32 MFMA, form 1 with polyphase Winograd conv2 / conv4 (shape form 2)"),
    ("cnn32_trunk_kernel<0, 8, false, 3>", "AffNet trunk, arith fp32_split3"),
    ("cnn32_trunk_kernel<0, 8, false, 2>", "AffNet trunk, arith fp32_split2h"),
    ("cnn32_trunk_kernel<1, 8, false, 0>", "OriNet trunk, exact fp32 MFMA"),
    ("cnn32_trunk_kernel<1, 8, false, 3>", "OriNet trunk, arith fp32_split3"),
    ("cnn32_trunk_kernel<1, 8, false, 2>", "OriNet trunk, arith fp32_split2h"),
    ("hardnet_head_kernel<64>", "HardNet head GEMM (64-patch tiles), exact"),
    ("hardnet_head_s3_kernel<64, 3>", "HardNet head GEMM (64-patch tiles), arith fp32_split3"),
    ("hardnet_head_s3_kernel<64, 2>", "HardNet head GEMM (64-patch tiles), arith fp32_split2h"),
    ("rowmin_dist_kernel<128>", "SNN matching: MFMA distance tiles with a running row minimum"),
    ("spv_score_kernel", "spatial verification: T x T scoring of the affine-frame hypotheses"),
    ("spv_lo_kernel", "spatial verification: fp64 local optimisation, one workgroup"),
    ("epi_solve_kernel", "epipolar verification: one 8-point solve per thread in fp64, the 8 x 9 system in LDS as [element][thread]"),
    ("epi_score_kernel", "epipolar verification: (T x rounds) x T scoring of the hypotheses by the Sampson error"),
    ("epi_lo_kernel", "epipolar verification: fp64 local optimisation (9 x 9 and 3 x 3 Jacobi in LDS), one workgroup"),
    ("epp_list_kernel", "plane-aware epipolar verification: centres and the stable compaction of the matches off the plane, one workgroup"),
    ("epp_hyp_kernel", "plane-aware epipolar verification: one plane-and-parallax hypothesis per thread in fp64, registers only"),
    ("epp_score_kernel", "plane-aware epipolar verification: (U x rounds) x T scoring by the shared Sampson body"),
    ("epp_refit_kernel", "plane-aware epipolar verification: fp64 refit of the epipole (3 x 3 Jacobi in LDS) and the decision, one workgroup"),
    ("guided_tile_kernel<0, 2, false>", "guided matching, planar model, forward pass: the matcher's distance tiles over one column chunk, two admissible neighbours per row and lane"),
    ("guided_tile_kernel<0, 1, true>", "guided matching, planar model, backward pass: the sides exchanged, one admissible neighbour"),
    ("guided_tile_kernel<1, 2, false>", "guided matching, epipolar model, forward pass"),
    ("guided_tile_kernel<1, 1, true>", "guided matching, epipolar model, backward pass"),
    ("guided_select_kernel", "guided matching: distance bound, ratio and mutual test, compaction in row order, one workgroup"),
    ("rowmin_many_kernel<128>", "SNN matching of many pairs per call: the same row-minimum body, pair index on the grid"),
    ("spv_many_score_kernel", "spatial verification of many pairs per call: the same scoring body, pair index on the grid"),
    ("spv_many_lo_kernel", "spatial verification of many pairs per call: the same fp64 local optimisation, one workgroup per pair"),
    ("epi_many_solve_kernel", "epipolar verification of many pairs per call: the same 8-point solve body, pair index on the grid"),
    ("epi_many_score_kernel", "epipolar verification of many pairs per call: the same scoring body, pair index on the grid"),
    ("epi_many_lo_kernel", "epipolar verification of many pairs per call: the same fp64 local optimisation, one workgroup per pair"),
    ("guided_many_tile_kernel<0, 2, false>", "guided matching of many pairs per call, planar model, forward pass: the same tile body, pair index on the grid"),
    ("guided_many_tile_kernel<0, 1, true>", "guided matching of many pairs per call, planar model, backward pass"),
    ("guided_many_tile_kernel<1, 2, false>", "guided matching of many pairs per call, epipolar model, forward pass"),
    ("guided_many_tile_kernel<1, 1, true>", "guided matching of many pairs per call, epipolar model, backward pass"),
    ("ratio_tile_kernel<2, false>", "ratio-test matching without a radius: the matcher's distance tiles over one column chunk, two neighbours per row and lane"),
    ("ratio_tile_kernel<1, false>", "ratio-test matching: the nearest column per row (forward pass with a radius) or the nearest row per column (backward pass)"),
    ("ratio_tile_kernel<1, true>", "ratio-test matching, FGINN pass: the first neighbour whose centre is inconsistent with the nearest column's"),
    ("ratio_select_kernel<true>", "ratio-test matching with a radius: the two slots to (n1, 2), distance bound, ratio and mutual test, compaction in row order"),
    ("ratio_select_kernel<false>", "ratio-test matching without a radius: distance bound, ratio and mutual test, compaction in row order, one workgroup"),
    ("ratio_many_tile_kernel<2, false, false>", "ratio-test matching of many pairs per call, no radius: the same tile body, pair index on the grid"),
    ("ratio_many_tile_kernel<1, false, false>", "ratio-test matching of many pairs per call: the nearest column per row"),
    ("ratio_many_tile_kernel<1, true, false>", "ratio-test matching of many pairs per call, FGINN pass"),
    ("ratio_many_tile_kernel<1, false, true>", "ratio-test matching of many pairs per call, backward pass"),
    ("knn_tile_kernel<128, 1>", "descriptor index, k = 1: the matcher's distance tiles over one column chunk, one neighbour per row and lane"),
    ("knn_tile_kernel<128, 2>", "descriptor index, k = 2: two neighbours per row and lane in registers"),
    ("knn_tile_kernel<128, 4>", "descriptor index, k = 3, 4: four neighbours per row and lane"),
    ("knn_tile_kernel<128, 8>", "descriptor index, k = 5 .. 8: eight neighbours per row and lane"),
    ("knn_merge_kernel<8>", "descriptor index: merge of a row's partial lists (the chunks', or the inverted file's probed cells'), one wavefront per query row (k = 5 .. 8)"),
    ("knn_vote_kernel", "descriptor index: one vote per (query row, image) behind the ratio gate"),
    ("q8_quantize_kernel", "descriptor index, int8: fp32 descriptors -> int8 rows and their sums of squares, 32 lanes per row"),
    ("knn_q8_tile_kernel<1, 4>", "descriptor index, int8, k = 1: i8 MFMA distance steps of 32 columns over one chunk, 256 query rows per workgroup"),
    ("knn_q8_tile_kernel<2, 4>", "descriptor index, int8, k = 2: two neighbours per row and lane, 256 query rows per workgroup"),
    ("knn_q8_tile_kernel<4, 2>", "descriptor index, int8, k = 3, 4: four neighbours per row and lane, 128 query rows per workgroup"),
    ("knn_q8_tile_kernel<8, 2>", "descriptor index, int8, k = 5 .. 8: eight neighbours per row and lane, 128 query rows per workgroup"),
    ("knn_q8_merge_kernel<8>", "descriptor index, int8: merge of the chunks' lists, one wavefront per query row (k = 5 .. 8)"),
    ("ivf_tile_kernel<1>", "descriptor index, inverted file, k = 1: 16 gathered query rows against one cell, the four waves split its 16-column tiles"),
    ("ivf_tile_kernel<2>", "descriptor index, inverted file, k = 2: two neighbours per row and lane"),
    ("ivf_tile_kernel<4>", "descriptor index, inverted file, k = 3, 4: four neighbours per row and lane"),
    ("ivf_tile_kernel<8>", "descriptor index, inverted file, k = 5 .. 8: eight neighbours per row and lane"),
    ("ivf_q8_tile_kernel<1>", "descriptor index, inverted file, int8, k = 1: 16 gathered query rows against one cell of int8 rows, the four waves split its 64-column steps"),
    ("ivf_q8_tile_kernel<2>", "descriptor index, inverted file, int8, k = 2: two neighbours per row and lane"),
    ("ivf_q8_tile_kernel<4>", "descriptor index, inverted file, int8, k = 3, 4: four neighbours per row and lane"),
    ("ivf_q8_tile_kernel<8>", "descriptor index, inverted file, int8, k = 5 .. 8: eight neighbours per row and lane"),
    ("ivf_scan_kernel", "descriptor index, inverted file: scan over the cells' pair counts, group starts and the table of work items, one workgroup"),
    ("ivf_cell_means_kernel", "descriptor index, inverted file: codebook update, one workgroup per cell, double sums in row order"),
    ("hessian_nms_kernel<5>", "Hessian + 3-D NMS + centroid, 5 levels per octave"),
    ("blur2d_kernel<13, 4>", "Gaussian blur 13 x 13, 64 x 64 tiles"),
    ("blur2d_pair_kernel<15, 9, 4>", "paired blur 15 x 15 / 9 x 9"),
    ("dense_conv_kernel<32, 32, 1", "dense AffNetFastFullConv conv3, exact"),
    ("dense_conv_s3_kernel<32, 32, 1, LayQ<16, 16, 18, 32, 0, 3>", "dense AffNetFastFullConv conv3, arith fp32_split3"),
    ("dense_conv_s3_kernel<32, 32, 1, LayR<16, 16, 20, 32", "dense AffNetFastFullConv conv3, arith fp32_split2h"),
]


def design_table(ks=None):
    ks = ks or all_kernels()
    lines = ["| kernel | role | VGPR | LDS bytes | scratch bytes | VGPR spills | workgroups / CU |", "|---|---|---|---|---|---|---|"]
    for pat, label in DESIGN_KERNELS:
        hit = [k for k in ks.values() if pat in k["demangled"]]
        if not hit:
            lines.append("| `%s` | %s | (not built) | | | | |" % (pat, label))
            continue
        k = hit[0]
        lines.append("| `%s` | %s | %d | %d | %d | %d | %d |" % (k["demangled"], label, k.get("vgpr_count", 0) + k.get("agpr_count", 0), k.get("group_segment_fixed_size", 0),
                                                             k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0), workgroups_per_cu(k)))
    return "\n".join(lines)


def main():
    ks = all_kernels()
    if "--json" in sys.argv:
        print(json.dumps(ks, indent=1, sort_keys=True))
        return
    if "--design" in sys.argv:
        print(design_table(ks))
        return
    print("| kernel | object | VGPR (+AGPR) | SGPR | LDS bytes | scratch bytes | VGPR spills | workgroups / CU (LDS, registers) |")
    print("|---|---|---|---|---|---|---|---|")
    for name in sorted(ks, key=lambda n: (ks[n]["object"], ks[n]["demangled"])):
        k = ks[name]
        print("| `%s` | %s | %d (+%d) | %d | %d | %d | %d | %d |" % (k["demangled"], k["object"], k.get("vgpr_count", 0), k.get("agpr_count", 0), k.get("sgpr_count", 0),
                                                              k.get("group_segment_fixed_size", 0), k.get("private_segment_fixed_size", 0),
                                                              k.get("vgpr_spill_count", 0), workgroups_per_cu(k)))


if __name__ == "__main__":
    main()
