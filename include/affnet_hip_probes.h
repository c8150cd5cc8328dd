/*
 * affnet_hip_probes.h - probe kernels of the tuning / measurement tools under tools/.
 *
 * NOT in libaffnet_hip.so: these entry points exist only in libaffnet_hip_probes.so = the product objects plus csrc/debug.hip, split_probe.hip
 * and cnn_probe.hip (`AFFNET_PROBES=1 bash affnet_amd/csrc/build.sh`; __graft_entry__.build() builds it next to the product library so that the tools
 * travel to the GPU box).  The tools select it with AFFNET_HIP_LIB=<path> (affnet_amd/_lib.py).  The shipped library holds product
 * kernels (+ the stamped debug instantiations of affnet_hip_debug.h) only.
 */
#ifndef AFFNET_HIP_PROBES_H
#define AFFNET_HIP_PROBES_H

#include "affnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning aid: runs the MFMA loop of one layer in isolation `reps` times per workgroup on `n_blocks` workgroups (same LDS
 * footprint as the trunk kernel).  layer 1 / 5: HardNet conv1 / conv5 (d_packed = HardNet's packed weights); 13 / 14 / 15:
 * AffNet conv3 as 2 x 2 tiles / conv3 as 4 x 1 tiles / conv5 (d_packed = AffNet's).  probe bit 0: no weight loads inside
 * the loop, bit 1: no activation loads, bit 2: accumulators in AGPRs, bit 3: lane-consecutive LDS read pattern (HardNet
 * layers only) - separates matrix-pipe issue efficiency from L2 / LDS effects.  d_out: 2 floats (sink). */
int affnet_cnn32_probe(const float* d_packed, int layer, int probe, int reps, int n_blocks, float* d_out, void* stream);

/* Counter calibration (MI355X_MICROARCH.md, HBM section: "calibrate on a known byte count in your own access pattern"):
 * streams exactly n_bytes (a multiple of 64 KiB) with `width` bytes per lane per load (4, 8 or 16), fully coalesced.
 *   mode 0: read d_src, reduce, one 4-byte store per workgroup to d_dst     (known READ bytes  = n_bytes)
 *   mode 1: write d_dst with a lane pattern, no reads                        (known WRITE bytes = n_bytes)
 *   mode 2: 64 x 64 fp32 tiles with a (halo)-pixel apron through LDS like the blur / Hessian tile loaders: image
 *           (n_bytes / 4 / 4096 rows of 4096 px), 4-byte loads, known unique bytes = n_bytes (halo re-reads hit L2)
 * Run under `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE`; tools/fetch_calib.py turns the counters into the per-width
 * factors that tools/pmc_traffic.py applies. */
int affnet_debug_stream(const void* d_src, void* d_dst, size_t n_bytes, int width, int mode, int halo, void* stream);

/* Numerics / rate probes of the split-operand arithmetic (AFFNET_ARITH_FP32_SPLIT3): fp32 operands as three bf16 terms on v_mfma_f32_16x16x32_bf16 (csrc/split_probe.hip).
 *   affnet_split3_gemm: d_C (M x N) = d_A (M x K) * d_Bt^T (d_Bt: N x K), M, N multiples of 16, K of 32.  mode 0 = the exact-fp32
 *     v_mfma_f32_16x16x4_f32 chain (today's arithmetic), 1 = six split terms, 2 = nine, 3 = the leading bf16 term only.
 *   affnet_split3_rate: sustained rate of the inner-loop shape a trunk layer would have (fragments from LDS, 4 pixel tiles x 1 channel
 *     tile); terms = 6 / 9 on bf16 MFMA, 1 = the fp32 16x16x4 loop over the same tiles.  One launch = n_blocks x 8 waves x reps x 4 tiles
 *     x (16 x 16 x 32) multiply-adds.  d_out: 2 floats (sink). */
int affnet_split3_gemm(const float* d_A, const float* d_Bt, int M, int N, int K, int mode, float* d_C, void* stream);
int affnet_split3_rate(int reps, int terms, int n_blocks, float* d_out, void* stream);

/* Read-back of the fused AffNet shape pass (affnet_set_shape_form) for the tests: where a bound context keeps, after affnet_describe_detected, the shape
 * matrices A of all candidates ([image][capacity_prefilter][4] floats) and the per-candidate flags of the margin rule ([image][capacity_prefilter] int32,
 * written for the candidates AffNet was evaluated on; forms AFFNET_SHAPE_FORM_WINOGRAD and _POLYPHASE only; the orientation and descriptor stages reuse that scratch, so
 * read them after a call with do_ori = 0 and no descriptors), and the candidates' normalised frames as the detector half
 * left them ([image][capacity_prefilter][6] floats; a test plants a non-finite frame there, which affnet_load_frames would refuse).  out[0] / out[1] / out[2]:
 * offsets from the workspace base, in 4-byte units.  Host only; the context may come from libaffnet_hip.so of the same build. */
int affnet_probe_shape_offsets(const affnet_ctx* ctx, int64_t out[3]);

/* Ledger of the workspace of a context (affnet_workspace_bytes), for the tests: one record per area, from the table that affnet_ctx_create sizes the
 * workspace from and affnet_bind_workspace takes its pointers from.  Records with parent < 0 are the carve units: in offset order, each on a 256-byte
 * boundary, tiling [0, affnet_workspace_bytes) with nothing but alignment padding between them.  A record with parent >= 0 is a view inside that unit
 * (offset still from the workspace base): the resp / syx (lafs) / ids arrays of a list lie back to back from the unit's start; the views of "cnn_scratch" are
 * a union - AffNet's head partials with the margin rule's flags behind them, OriNet's head partials, HardNet's conv5 tensor with the split-K partials
 * behind it - used one after the other.  kind: the element type (AFFNET_WS_RECORDS: the detector's 32-byte raw maxima; AFFNET_WS_GROUP: a unit of mixed
 * kinds, see its views).  cleared: 1 when the detector half of every fused call clears the area itself; every other area holds what the call's kernels wrote
 * (DESIGN.md section 3 says who, and why no read comes first).  Writes min(max, n) records and returns n, the number of records; < 0: an AFFNET_ERR_* code.
 * Host only; the context need not be bound and may come from libaffnet_hip.so of the same build. */
enum { AFFNET_WS_F32 = 0, AFFNET_WS_I32 = 1, AFFNET_WS_U8 = 2, AFFNET_WS_RECORDS = 3, AFFNET_WS_GROUP = 4 };
typedef struct affnet_ws_area {
    char name[40];
    int64_t offset, bytes;
    int32_t kind, cleared, parent, reserved;
} affnet_ws_area;
int affnet_probe_workspace_areas(const affnet_ctx* ctx, int max, affnet_ws_area* out);

/* Layer dump of the Winograd AffNet trunk (conv1 / conv3 / conv5 as F(2x2, 3x3): what shape form AFFNET_SHAPE_FORM_WINOGRAD runs on every candidate), for the
 * tests: affnet_cnn32_debug_layer's arguments and output (the activations after trunk layer `layer` = 0 .. 5 of the one 32 x 32 patch, [channel][y][x]), which
 * always answers with the direct trunk for AffNet.  net_kind must be AFFNET_NET_AFFNET, the context in AFFNET_ARITH_FP32_MFMA; it may come from
 * libaffnet_hip.so of the same build. */
int affnet_probe_affnet_wino_layer(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream);

/* The same trunk on n <= 65535 patches (n, 32, 32), for tools/cnn_phase_timing.py: leaves the head partials ([patch][8 waves][4] floats) in d_partials, no finish
 * kernel; writes the phase stamps when the context has a stamp buffer (affnet_cnn32_debug_timing). */
int affnet_probe_affnet_wino_partials(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_partials, void* stream);

/* The same two for the first trunk of shape form AFFNET_SHAPE_FORM_POLYPHASE (the Winograd AffNet trunk with conv2 / conv4 as polyphase Winograd F(2x2, 2x2)), and
 * _u: the derived polyphase weights of layer 2 (25 x 16 x 32 floats) or 4 (25 x 32 x 64) of an AffNet or OriNet blob, in the order the kernels read them (the exact
 * OriNet trunk, which affnet_cnn32_forward / affnet_cnn32_debug_layer run, reads the same sections of its own blob). */
int affnet_probe_affnet_poly_layer(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream);
int affnet_probe_affnet_poly_partials(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_partials, void* stream);
int affnet_probe_trunk16_poly_u(affnet_ctx* ctx, int net_kind, const float* d_packed, int layer, float* d_out, void* stream);

/* The exact HardNet trunk of descriptor form AFFNET_DESC_FORM_POLYPHASE (conv2 / conv4 as polyphase Winograd F(2x2, 2x2)) on patch tensors, which no entry point of
 * the product library runs (affnet_cnn32_forward always answers with form 0).  The context must be in AFFNET_ARITH_FP32_MFMA; it may come from libaffnet_hip.so of
 * the same build.
 *   _layer:   affnet_cnn32_debug_layer's arguments and output for the one 32 x 32 patch (layer 0 .. 5, [channel][y][x]);
 *   _forward: affnet_cnn32_forward's for n patches (d_out (n, 128) descriptors, d_scratch n * (8192 + 512) floats); writes the phase stamps when the context
 *             has a stamp buffer (affnet_cnn32_debug_timing);
 *   _u:       the derived weights of layer 2 (25 x 32 x 64 floats) or 4 (25 x 64 x 128), in the order the kernel reads them. */
int affnet_probe_hardnet_poly_layer(affnet_ctx* ctx, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream);
int affnet_probe_hardnet_poly_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, float* d_scratch, void* stream);
int affnet_probe_hardnet_poly_u(affnet_ctx* ctx, const float* d_packed, int layer, float* d_out, void* stream);

/* The same three for descriptor form AFFNET_DESC_FORM_F43 (form 1 with conv3 as Winograd F(4x4, 3x3)); _u: the derived F(4x4, 3x3) weights of layer 1 (36 x 32 x 32
 * floats; derived, though the trunk runs conv1 as F(2x2, 3x3)) or 3 (36 x 64 x 64), in the order the kernel reads them. */
int affnet_probe_hardnet_f43_layer(affnet_ctx* ctx, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream);
int affnet_probe_hardnet_f43_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, float* d_scratch, void* stream);
int affnet_probe_hardnet_f43_u(affnet_ctx* ctx, const float* d_packed, int layer, float* d_out, void* stream);

/* Descriptor form AFFNET_DESC_FORM_F43_CONV5 (form 2 with conv5 as Winograd F(4x4, 3x3) in a kernel of its own, four patches per workgroup):
 *   _trunk_layer: affnet_cnn32_debug_layer's arguments and output for layers 0 .. 4 of its trunk kernel;
 *   _forward:     as affnet_probe_hardnet_f43_forward; with a stamp buffer the conv5 kernel writes stamps 24 .. 31 into the record of the first patch of every group of four;
 *   _layer:       the conv5 kernel alone, in place on n slots of 8192 floats: conv4's post-ReLU tensor as [c / 4][pixel][c % 4] in, conv5's post-ReLU tensor as
 *                 [pixel][channel] out (the order the head GEMM reads); groups of four consecutive slots, the last may hold 1 .. 3;
 *   _u:           the derived F(4x4, 3x3) weights of layer 5 (36 x 128 x 128 floats), in the order the kernel reads them. */
int affnet_probe_hardnet_c5_trunk_layer(affnet_ctx* ctx, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream);
int affnet_probe_hardnet_c5_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, float* d_scratch, void* stream);
int affnet_probe_hardnet_c5_layer(affnet_ctx* ctx, const float* d_packed, float* d_slots, int n, void* stream);
int affnet_probe_hardnet_c5_u(affnet_ctx* ctx, const float* d_packed, float* d_out, void* stream);

/* Descriptor form AFFNET_DESC_FORM_F43_CONV1 (form 3 with conv0 + conv1 streamed, conv1 as Winograd F(4x4, 3x3)):
 *   _trunk_layer: affnet_cnn32_debug_layer's arguments and output for layers 1 .. 4 of its trunk kernel (layer 0 never exists as a tensor: refused);
 *   _forward:     as affnet_probe_hardnet_c5_forward.
 * conv1's derived weights are affnet_probe_hardnet_f43_u's layer 1. */
int affnet_probe_hardnet_c1_trunk_layer(affnet_ctx* ctx, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream);
int affnet_probe_hardnet_c1_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, float* d_scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AFFNET_HIP_PROBES_H */
