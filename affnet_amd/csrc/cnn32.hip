// 32x32-patch CNNs (AffNetFast / OriNetFast / HardNet) for gfx950 on the fp32 matrix cores.
//
// Replaces architectures.py:204-252 (AffNetFast), :33-82 (OriNetFast), HardNet.py:61-101
// (HardNet) incl. input_norm, eval-mode BatchNorm (folded into weights + bias at pack time),
// ReLU, the heads, rectifyAffineTransformationUpIsUp (LAF.py:285-291), get_rotation_matrix
// (LAF.py:276-283) and L2Norm (HardNet.py:12-19).
//
// Design (one workgroup = 8 wavefronts = one patch, whole trunk resident on the CU; details in DESIGN.md section 4):
//   * the patch is sampled from the pyramid (or loaded), standardised (mean / unbiased std + 1e-7, DPP wave reductions)
//     and stored as a zero-haloed 34 x 34 LDS tile;
//   * the exact path runs all six convolutions on v_mfma_f32_16x16x4_f32 (exact fp32): conv0 with K = 9 taps padded to 12 and the
//     accumulators initialised with the bias; the direct layers (conv2 / conv4 of every net, AffNet conv1..5) as implicit GEMMs
//     (cnn_mfma.h: conv3x3_mfma) with the WEIGHTS as the MFMA A operand and the ACTIVATIONS as the B operand, so a lane ends up with 4
//     consecutive channels of one pixel; the stride-1 layers as Winograd F(2x2, 3x3), U = G g G^T: HardNet's conv1 / conv3
//     (conv3x3_wino_mfma_pair_rows: two channel blocks share one window transform, one row of four transform positions per step, the next
//     step's reads and transform between this step's MFMAs) and conv5 (conv3x3_wino_mfma_shared_v: V shared through LDS), U from the blob;
//     OriNet's conv1 / conv3 (conv3x3_wino_mfma_rows, one row of four transform positions at a time on 128 registers; U derived from the
//     blob's taps by wino_derive_u_kernel in front of every launch) and conv5 (conv3x3_wino_mfma_half_rows: a wave pair per channel block, two position rows
//     each, one row exchanged through LDS in a fixed order, 2x2-pixel fragments straight into the head's LDS copy).  AffNet stays in the direct form:
//     the shape filter behind it turns on the last bits of its output, and another rounding changes which keypoints come back.  The
//     split-operand modes (affnet_set_arith) run conv1..5 on bf16 / fp16 terms (conv3x3_mfma_s3q);
//   * activations live in ONE LDS buffer, channel-interleaved by 4 ((c/4)*PSG + pixel*4 + c%4): one ds_read_b128 per lane =
//     the activation operands of four k-steps, one ds_write_b128 per tile in the epilogue (bias + ReLU), written IN PLACE
//     over the layer's input after a barrier.  No HBM traffic between layers;
//   * packed weights (weights_layout.h: w_tap_index; packed on the host by weights_pack.hip) stream from L2 through a buffer descriptor
//     (one buffer_load_dwordx4 per lane = the weight operands of four k-steps), software-pipelined one chunk ahead, loads interleaved
//     between the MFMAs;
//   * heads: HardNet stores its conv5 tile [pixel][channel] to HBM and an 8192 x 128 split-K MFMA GEMM over all patches
//     (hardnet_head_kernel + hardnet_finish_kernel: BN bias + L2 norm) follows; AffNet / OriNet reduce their heads' dot
//     products per wave straight from the conv5 accumulators (head_partials, head_partials_ori_lds) and affnet_finish_kernel /
//     orinet_finish_kernel combine the eight partials per patch in fixed order (tanh, rectification / atan2).
// Host side (end of the file): every entry point fills a CnnCall and cnn_launch runs cnn_check -> trunk_launch -> finish_affnet /
// finish_orinet / hardnet_head; the prototypes other files call are in common.h.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "common.h"

#include "cnn_mfma.h"
#include "shape_filter.h"

// AffNet head, first half, straight from the conv5 accumulators (no conv5 tensor in HBM): a lane owns channels c4..c4+3 of pixel p of
// each of its tiles = one float4 of the head weights [o][pixel][channel]; it forms its share of the 3 outputs (conv 64 -> 3, 8x8 valid,
// architectures.py:227-229), the wave reduces them and lane 0 writes the wave's partial sums to part[wave][4].  The eight partials per
// patch are combined in fixed order by affnet_finish_kernel (bit-reproducible, no atomics).  OriNet's head (2 x 9 outputs, part[8][18]):
// head_partials_ori_lds below.
#define HEAD_PART_AFF 32
#define HEAD_PART_ORI 144
template <int TM>
__device__ __forceinline__ void head_partials(const float* __restrict__ hw, const f32x4 (&bias)[1], const f32x4 (&acc)[TM][1],
                                              float* __restrict__ part, int wave, int lane) {
    constexpr int MT = 4, MG = MT / TM;
    const int mg = wave % MG, ng = wave / MG;
    const int n = lane & 15, g = lane >> 4;
    const int c4 = ng * 16 + 4 * g;
    f32x4 v[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        v[i] = acc[i][0] + bias[0];
        v[i].x = fmaxf(v[i].x, 0.0f); v[i].y = fmaxf(v[i].y, 0.0f); v[i].z = fmaxf(v[i].z, 0.0f); v[i].w = fmaxf(v[i].w, 0.0f);
    }
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(hw, 3 * 4096);
    f32x4 w[3][TM];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int i = 0; i < TM; ++i) w[o][i] = buf_read4(r, (n * 64 + c4) * 4, (o * 4096 + (mg * TM + i) * 16 * 64) * 4);
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        float sacc = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) sacc = fmaf(v[i][j], w[o][i][j], sacc);
        sacc = wave_sum(sacc);
        if (lane == 0) part[wave * 4 + o] = sacc;
    }
}

// OriNet head through LDS (round 4).  The direct form (as in head_partials) made every lane fetch the weight vector of each of the 2 x 9 (output, tap)
// pairs for its own pixel: 36 buffer_load_dwordx4 per wave, 295 KB of L2 -> L1 traffic per patch for 32 KB of distinct weights - the head
// took 14.4 k cycles per workgroup against AffNet's 3.3 k (tools/s3_phase_timing.py), L1-bound.  Here the roles are swapped: a lane owns
// the WEIGHT position (ky, kx) = its tile pixel and 4 channels, loads those weights once per output (4 loads) and reads the nine shifted
// ACTIVATIONS from a zero-haloed 10 x 10 copy of the conv5 output in LDS (the activation buffer is dead after the conv5 loop):
//   out[o][qy][qx] = sum over (ky, kx, c) of  W[o][ky][kx][c] * A[qy + ky - 1][qx + kx - 1][c]      (A = 0 outside the 8 x 8 map)
// Same products as before, grouped by weight position instead of activation position; same [wave][o * 9 + q] partial layout.
#define ORI_HP 68        // floats per pixel of the LDS copy (64 channels + 4: consecutive pixels 4 banks apart)
// The head's two halves for the Winograd conv5 of the exact trunk.  First half: the conv5 output (bias + ReLU) into the zero-haloed 10 x 10 copy -
// ori_head_zero_halo, and the loop's 2 x 2-pixel fragments through wino5_store_lds (cnn_mfma.h).  Second half: ori_head_reduce, lane-owned weights
// (ori_head_weights, requested ahead of the barriers) against the nine shifted activations, after a barrier.
struct OriHeadLane {     // the lane's weight position: pixel n of tiles mg * TM + i, channels c4 .. c4 + 3
    int mg, n, c4;
    template <int TM>
    __device__ __forceinline__ static OriHeadLane of(int wave, int lane) {
        constexpr int MT = 4, MG = MT / TM;
        const int mg = wave % MG, ng = wave / MG;
        const int n = lane & 15, g = lane >> 4;
        return {mg, n, ng * 16 + 4 * g};
    }
};
template <int TM>
__device__ __forceinline__ void ori_head_weights(const float* __restrict__ hw, const OriHeadLane& L, f32x4 (&w)[2][TM]) {
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(hw, 2 * 4096);
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int i = 0; i < TM; ++i) w[o][i] = buf_read4(r, (L.n * 64 + L.c4) * 4, (o * 4096 + (L.mg * TM + i) * 16 * 64) * 4);
}
template <int NTHR>
__device__ __forceinline__ void ori_head_zero_halo(float* act, int tid) {
    for (int e = tid; e < 36 * 16; e += NTHR) {                          // zero halo of the 10 x 10 grid: 36 pixels x 16 float4
        const int hp = e >> 4, q4 = e & 15;
        const int y = hp < 10 ? 0 : (hp < 20 ? 9 : 1 + ((hp - 20) >> 1)), x = hp < 10 ? hp : (hp < 20 ? hp - 10 : ((hp - 20) & 1) * 9);
        *reinterpret_cast<f32x4*>(&act[(y * 10 + x) * ORI_HP + 4 * q4]) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
}
template <int TM>
__device__ __forceinline__ void ori_head_pbase(const OriHeadLane& L, int (&pbase)[TM]) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int p = (L.mg * TM + i) * 16 + L.n;
        pbase[i] = ((p >> 3) * 10 + (p & 7)) * ORI_HP + L.c4;           // (ky, kx) in padded coordinates of tap q = (0, 0)
    }
}
template <int TM>
__device__ __forceinline__ void ori_head_reduce(const f32x4 (&w)[2][TM], const int (&pbase)[TM], float* __restrict__ part, const float* act, int wave, int lane) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(&act[pbase[i] + ((q / 3) * 10 + q % 3) * ORI_HP]);
#pragma unroll
            for (int j = 0; j < 4; ++j) { s0 = fmaf(av[j], w[0][i][j], s0); s1 = fmaf(av[j], w[1][i][j], s1); }
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) { part[wave * 18 + q] = s0; part[wave * 18 + 9 + q] = s1; }
    }
}
// The direct form's head in one piece (the split-operand OriNet trunks): both halves as above, kept as one body so that those kernels' code does not move.
template <int TM, int NTHR>
__device__ __forceinline__ void head_partials_ori_lds(const float* __restrict__ hw, const f32x4 (&bias)[1], const f32x4 (&acc)[TM][1],
                                                      float* __restrict__ part, float* act, int wave, int lane, int tid) {
    constexpr int MT = 4, MG = MT / TM;
    const int mg = wave % MG, ng = wave / MG;
    const int n = lane & 15, g = lane >> 4;
    const int c4 = ng * 16 + 4 * g;
    f32x4 v[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        v[i] = acc[i][0] + bias[0];
        v[i].x = fmaxf(v[i].x, 0.0f); v[i].y = fmaxf(v[i].y, 0.0f); v[i].z = fmaxf(v[i].z, 0.0f); v[i].w = fmaxf(v[i].w, 0.0f);
    }
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(hw, 2 * 4096);
    f32x4 w[2][TM];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int i = 0; i < TM; ++i) w[o][i] = buf_read4(r, (n * 64 + c4) * 4, (o * 4096 + (mg * TM + i) * 16 * 64) * 4);
    __syncthreads();                                                     // every wave has finished reading the conv5 input from `act`
    for (int e = tid; e < 36 * 16; e += NTHR) {                          // zero halo of the 10 x 10 grid: 36 pixels x 16 float4
        const int hp = e >> 4, q4 = e & 15;
        const int y = hp < 10 ? 0 : (hp < 20 ? 9 : 1 + ((hp - 20) >> 1)), x = hp < 10 ? hp : (hp < 20 ? hp - 10 : ((hp - 20) & 1) * 9);
        *reinterpret_cast<f32x4*>(&act[(y * 10 + x) * ORI_HP + 4 * q4]) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int pbase[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int p = (mg * TM + i) * 16 + n;
        pbase[i] = ((p >> 3) * 10 + (p & 7)) * ORI_HP + c4;             // (ky, kx) in padded coordinates of tap q = (0, 0)
        *reinterpret_cast<f32x4*>(&act[pbase[i] + 11 * ORI_HP]) = v[i];  // interior pixel (py + 1, px + 1)
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(&act[pbase[i] + ((q / 3) * 10 + q % 3) * ORI_HP]);
#pragma unroll
            for (int j = 0; j < 4; ++j) { s0 = fmaf(av[j], w[0][i][j], s0); s1 = fmaf(av[j], w[1][i][j], s1); }
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) { part[wave * 18 + q] = s0; part[wave * 18 + 9 + q] = s1; }
    }
}

struct PyrSrc {            // pyramid sampling source (fused sampler)
    PyrTable t;            // the samplers' level table (common.h)
    float base[32];        // affine_grid base coordinates for PS = 32
};

struct CnnArgs {
    const float* packed;
    NetOffsets off;
    const float* wino_u;   // exact OriNet: U = G g G^T of conv1, conv3 and conv5, derived from the blob in front of this launch (wino_derive_u_kernel)
    const float* patches;  // (n,32,32) or NULL -> sample from the pyramid
    const float* lafs;     // normalised LAFs when sampling
    const int32_t* ids;    // (octave, level, *) when sampling
    const int32_t* count;
    int n_max;
    float* out;            // AffNet/OriNet: (n,2,2); HardNet: trunk output (n,8192)
    int dbg_layer;         // >= 0: dump activations after this trunk layer of patch 0 and exit
    int s3_alt;            // tuning variant bits of the split-operand trunks (affnet_debug_split3_variant): bit 0 = the two waves of a SIMD alternate at the higher priority inside the HardNet loops
    float* dbg_out;
    unsigned long long* dbg_time;   // != NULL: s_memtime stamps [patch][wave][32] at the phase boundaries (tuning aid)
    // Row window [row_begin, row_begin + gridDim.x) of every image, and the lazy-evaluation predicate of the fused pipeline: when
    // skip_cnt != NULL the launch does nothing for an image whose detections are response-sorted (CNT_SEL_MODE == 1) and whose first
    // pass already produced skip_n survivors of the shape filter (CNT_SURVIVED1) - pipeline.hip, affnet_describe_detected.
    int row_begin;
    const int32_t* skip_cnt;
    int skip_n;
    // Shape-stage bookkeeping done by thread 0 of workgroup (0, image) of the AffNet trunk launches (each was a 5 us launch of its
    // own): shape_op 1 = first pass: survivor / evaluation counters = 0; 2 = second (lazy) pass: freeze the first pass's survivor
    // count (CNT_SURVIVED1) for the predicate of the finish + filter kernel that follows this launch.  The trunk workgroups
    // themselves test CNT_SURVIVED, which nothing changes while a trunk launch runs.
    int32_t* shape_cnt;
    int shape_op;
};
// (the split-operand variants are template instantiations: cnn32_trunk_kernel<KIND, NW, STAMPS, S3>, S3 = 3 bf16 terms or 2 fp16 terms; 0 = exact)

__device__ __forceinline__ bool lazy_skip(const int32_t* skip_cnt, int skip_n, int image, int which = CNT_SURVIVED1) {
    if (!skip_cnt) return false;
    const int32_t* c = skip_cnt + (size_t)image * CNT_TOTAL;
    return c[CNT_SEL_MODE] == 1 && c[which] >= skip_n;
}

#define CNN_STAMP(k)                                                                                     \
    do {                                                                                                 \
        if (STAMPS && a.dbg_time && lane == 0) a.dbg_time[((size_t)pidx * NW + wave) * 32 + (k)] = __builtin_readcyclecounter(); \
    } while (0)

// U = G g G^T of the Winograd layers of the exact OriNet trunk (conv1 16 -> 16, conv3 32 -> 32, conv5 64 -> 64; the AffNet blob has the same shapes and the debug accessor derives it too), in w_tap_index order like NetLayout::w_wino.
// Not part of the blob (its size and hash are pinned, and a blob packed by an older library stays valid): derived on the device from the blob's
// BN-folded fp32 taps into a buffer the context owns, one region per net kind.
struct Wino16 {
    static constexpr int U1 = 16 * 16 * 16, U3 = 16 * 32 * 32, U5 = 16 * 64 * 64, FLOATS = U1 + U3 + U5;   // floats per net
    static constexpr int PAIRS = 16 * 16 + 32 * 32 + 64 * 64;                        // (cin, cout) pairs of the three layers
    static constexpr int NB1 = 2, NB3 = 1;                                           // (tile block, channel block) passes per wave: 16 x 1 / 8, 4 x 2 / 8
    static constexpr int offset(int layer) { return layer == 1 ? 0 : (layer == 3 ? U1 : U1 + U3); }
    static constexpr int floats(int layer) { return layer == 1 ? U1 : (layer == 3 ? U3 : U5); }
};

// One thread per (cin, cout) pair of conv1 (256), conv3 (1024) and conv5 (4096), numbered in the fragment order (so that a wave's loads and stores are contiguous): reads its
// 9 taps and writes its 16 transform positions, both in w_tap_index order; the transform and its operation order are wino_weight_transform's (weights_layout.h).
__global__ __launch_bounds__(256) void wino_derive_u_kernel(const float* __restrict__ packed, int w1, int w3, int w5, float* __restrict__ U) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Wino16::PAIRS) return;
    const int l = e >= 256 + 1024 ? 5 : (e >= 256 ? 3 : 1);
    const int ch = 8 << ((l + 1) >> 1);                                 // cin == cout: 16, 32, 64
    const float* src = packed + (l == 5 ? w5 : (l == 3 ? w3 : w1));
    float* dst = U + Wino16::offset(l);
    e -= l == 5 ? 256 + 1024 : (l == 3 ? 256 : 0);
    const int n = (e >> 2) % ch, c = (e >> 2) / ch * 4 + (e & 3);       // e == w_tap_index(0, c, n, ch, ch)
    float g[9], u[16];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = src[w_tap_index(t, c, n, ch, ch)];
    wino_weight_transform(g, u);
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) dst[w_tap_index(xi, c, n, ch, ch)] = u[xi];
}

template <int CB>
struct TrunkLds {
    static constexpr int ACT = (CB / 4) * LayC0::PSG;   // the largest layout (conv0 output); all later ones are smaller
    static constexpr int PATCH = WP32 * WP32;
    static constexpr int RED = 256;                     // reduction slots (block_sum, head exchanges)
    static constexpr int TOTAL = ACT + PATCH + RED;
};

// Per-net constants of the trunk: CB channels after conv0, NW wavefronts, per-wave register blocking (TM x TN tiles of 16 px x 16 ch;
// MG * NG == NW for every layer) and plane groups per pipeline chunk of the direct-form layers.
template <int KIND, int NW>
struct TrunkShape {
    static constexpr int CB = (KIND == AFFNET_NET_HARDNET) ? 32 : 16;
    static constexpr int NTHR = NW * 64;
    static constexpr int T1M = (CB == 16) ? 8 : 64 / NW, T1N = CB / 16;
    // conv2 / conv3: ONE channel tile per wave and as many pixel tiles as that allows - activation fragments come from LDS
    // (nearly free), weight fragments are 1 KB global loads whose cost shows in the MFMA rate: 4 x 1 instead of 2 x 2 took the
    // isolated AffNet conv3 loop from 121 to 146 TFLOP/s (tools/clock_probe.py 13 / 14)
    static constexpr int T2M = (CB == 16) ? 4 : 64 / NW, T2N = 1;
    static constexpr int T4M = (CB == 16) ? 2 : 32 / NW, T4N = 1;
    // plane groups (4 k-steps each) per pipeline chunk; VGPR budget 128 at 4 waves / SIMD, 256 at 2
    static constexpr int AREG = (NW == 8 && CB == 32) ? 128 : 48;
    static constexpr int G2 = pick_groups(CB, T2M, T2N, 32, AREG), G3 = pick_groups(2 * CB, T2M, T2N, 32, AREG);
    static constexpr int G4 = pick_groups(2 * CB, T4M, T4N, 32, AREG), G5 = pick_groups(4 * CB, T4M, T4N, 32, AREG);
};

template <int C, typename L, int NTHR>
__device__ __forceinline__ void dump_planes(const float* act, float* dst) {
    constexpr int H = L::H;
    for (int i = threadIdx.x; i < C * H * H; i += NTHR) {
        const int c = i / (H * H), r = i - c * H * H, y = r / H, x = r - y * H;
        dst[i] = act[L::at(c, y, x)];
    }
}

// Activation layouts of the split-operand flows of cnn32_trunk_kernel.  Three bf16 terms: term-interleaved 48-byte cells (LayQ), conv0 .. conv2 in two
// half-patch passes; two fp16 terms (AFFNET_ARITH_FP32_SPLIT2H): 16-byte pixels, the two terms of a row side by side (LayR; per-reader row
// pitch / group stride), conv0 once for the whole patch.
template <int CB>
struct SplitLays {
    typedef LayQ<16, 32, 34, CB, 0, 3> LQH;                      // three terms: conv0 output of half a patch, pre-split; read by conv1 (stride 1)
    typedef LayQ<16, 32, 34, CB, 16, 3> LQH2;                    // three terms: conv1 output of half a patch; read by conv2 at stride 2
    // two-term arithmetic: LayR's 16-byte pixels hold conv0's / conv1's output of the WHOLE patch (145 KB for 32 channels, 72.5 KB for 16), so conv0 runs once; conv1 / conv2
    // keep their two half-patch LOOPS (same register blockings) on 16-row views of the whole layouts - no second conv0 pass, no halo-row fix-ups between the halves
    using LR0 = LayR<32, 32, 34, CB, 0>;                          // conv0 output, read by conv1 (stride 1)
    using LR0H = LayR<16, 32, 34, CB, 0, 34>;                     // its 16-row view
    using LR1 = LayR<32, 32, 34, CB, 16>;                         // conv1 output, read by conv2 at stride 2
    using LR1H = LayR<16, 32, 34, CB, 16, 34>;
    static_assert(LR0::BYTES <= TrunkLds<CB>::ACT * 4 && LR1::BYTES <= TrunkLds<CB>::ACT * 4 && LR0H::GS == LR0::GS && LR1H::GS == LR1::GS, "whole-patch split layouts");
    static_assert(LQH::BYTES <= TrunkLds<CB>::ACT * 4 && LQH2::BYTES <= TrunkLds<CB>::ACT * 4, "pre-split layouts must fit the activation buffer");
};

// One workgroup = one patch through one trunk.  KIND: 0 AffNet, 1 OriNet, 2 HardNet (CB = 16 / 16 / 32); NW = 8 wavefronts; S3 = 0 exact,
// 3 / 2 = terms of the split-operand arithmetic.  After the prologue that all flows share (counters, lazy skip, priority, conv0 weights, input phase) the
// kernel is one straight-line body per flow: exact HardNet (Winograd), exact AffNet / OriNet, split HardNet, split AffNet / OriNet.  Every
// layer: MFMA loop -> request the next layer's first weight chunk and bias -> barrier (all waves done reading the input) -> zero the halo of
// the OUTPUT layout, bias + ReLU + store in place -> barrier.  No HBM traffic between layers.
// AffNet / OriNet: 79 KB LDS -> 2 workgroups per CU (4 waves / SIMD, 128 VGPRs); HardNet: 154 KB LDS -> 1 workgroup per
// CU (2 waves / SIMD, 256 VGPRs).
// STAMPS = debug instantiation: the s_memtime phase stamps of tools/cnn_phase_timing.py and the per-layer activation dumps
// of affnet_cnn32_debug_layer exist only there (26 stamp sites = 26 predicated stores + branches in every wave otherwise).
template <int KIND, int NW, bool STAMPS, int S3 = 0>
__global__ __launch_bounds__(NW * 64, (KIND == AFFNET_NET_HARDNET) ? NW / 4 : 4) void cnn32_trunk_kernel(CnnArgs a, PyrSrc ps) {
    static_assert(S3 == 0 || S3 == 2 || S3 == 3, "S3 = number of terms of the split arithmetic");
    using S = TrunkShape<KIND, NW>;
    constexpr int CB = S::CB, NTHR = S::NTHR;
    static_assert((CB / 4) * LayC1::PSG <= TrunkLds<CB>::ACT && (CB / 2) * LayC3::PSG <= TrunkLds<CB>::ACT, "LDS layout");
    __shared__ __attribute__((aligned(16))) float lds[TrunkLds<CB>::TOTAL];
    float* act = lds;
    float* patch = lds + TrunkLds<CB>::ACT;
    float* red = patch + TrunkLds<CB>::PATCH;
    // grid = (n_max, batch): row blockIdx.x of image blockIdx.y; global row = image * n_max + row
    const int n = a.count ? min(a.count[blockIdx.y], a.n_max) : a.n_max;
    const int prow = blockIdx.x + a.row_begin;
    if (KIND == AFFNET_NET_AFFNET && a.shape_cnt && blockIdx.x == 0 && threadIdx.x == 0) {
        int32_t* c = a.shape_cnt + (size_t)blockIdx.y * CNT_TOTAL;
        if (a.shape_op == 1) { c[CNT_SURVIVED] = 0; c[CNT_SURVIVED1] = 0; c[CNT_AFF_EVAL] = 0; }
        else if (a.shape_op == 2) c[CNT_SURVIVED1] = c[CNT_SURVIVED];
    }
    if (prow >= n || lazy_skip(a.skip_cnt, a.skip_n, blockIdx.y, CNT_SURVIVED)) return;
    const size_t pidx = (size_t)blockIdx.y * a.n_max + prow;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // Issue priority (HardNet only, one workgroup per CU): the short latency-bound phases (input, conv0, epilogues) run at
    // priority 3, the MFMA loops at 0: +2% (130 -> 133 TFLOP/s).  For AffNet / OriNet (two workgroups per CU) it is
    // zero-sum: the non-MFMA phases of one workgroup get 2x faster (with equal priorities the arbiter prefers the OLDER
    // waves, so a young workgroup next to an older one in its MFMA loop crawls: 3.7k vs 0.5k cycles per block reduction),
    // but their VALU instructions then displace the other workgroup's MFMA issue slots (-5% overall), so it stays off.
    if (KIND == AFFNET_NET_HARDNET) __builtin_amdgcn_s_setprio(3);
    CNN_STAMP(0);
    if (STAMPS && a.dbg_time && lane == 0) {   // where this workgroup runs (tuning aid: per-CU timelines)
        a.dbg_time[((size_t)pidx * NW + wave) * 32 + 14] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
        a.dbg_time[((size_t)pidx * NW + wave) * 32 + 15] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
    }
    // conv0 taps + bias (and for exact AffNet the first weight chunk, for exact OriNet the first U fragments of conv1): requested now, consumed after the input phase
    float w0[3][S::T1N];
    f32x4 bias0[S::T1N];
    conv0_load_w<NW, CB, S::T1M, S::T1N>(a.packed + a.off.w[0], a.packed + a.off.b[0], w0, bias0, wave, lane);
    f32x4 b1[1][S::T1N];
    f32x4 Ur[4];                                                      // exact OriNet: the rolling U register set of conv1 / conv3 / conv5
    if constexpr (S3 == 0 && KIND == AFFNET_NET_AFFNET) prefetch_b0<NW, CB, 32, S::T1M, S::T1N, 1>(a.packed + a.off.w[1], b1, wave, lane);
    if constexpr (S3 == 0 && KIND == AFFNET_NET_ORINET) wino_prefetch_u_row<NW, CB, CB, 32, Wino16::NB1>(a.wino_u, Ur, wave, lane);

    // ---- input: load or sample 1024 pixels (PPT per thread), standardise, store padded ----------------
    constexpr int PPT = 1024 / NTHR;                    // input pixels per thread (2 or 1)
    constexpr int RPT = 32 / PPT;                       // patch rows covered by one pass of the workgroup
    float v[PPT];
    if (a.patches) {
        const float* src = a.patches + pidx * 1024;
#pragma unroll
        for (int q = 0; q < PPT; ++q) v[q] = src[tid + q * NTHR];
    } else {
        int o = a.ids[3 * pidx], l = a.ids[3 * pidx + 1];
        o = o < 0 ? 0 : (o >= ps.t.n_octaves ? ps.t.n_octaves - 1 : o);
        l = l < 0 ? 0 : (l >= ps.t.n_levels ? ps.t.n_levels - 1 : l);
        const float* img = ps.t.lvl[o][l] + blockIdx.y * ps.t.img_stride;
        const int h = ps.t.h[o], w = ps.t.w[o];
        const float* L = a.lafs + 6 * pidx;
        const float m = (float)(h < w ? h : w);
        const float t00 = L[0] * m, t01 = L[1] * m, t02 = L[2] * (float)w;
        const float t10 = L[3] * m, t11 = L[4] * m, t12 = L[5] * (float)h;
#pragma unroll
        for (int q = 0; q < PPT; ++q)
            v[q] = aff_sample_bilinear(img, h, w, t00, t01, t02, t10, t11, t12, ps.base[tid & 31], ps.base[(tid >> 5) + q * RPT]);
    }
    CNN_STAMP(16);
    // halo of the padded patch (4 x 33 cells) and of the activation planes; interiors are written below / by conv0
    if (tid < 4 * 33) {
        const int e = tid;
        const int y = e < 34 ? 0 : (e < 68 ? 33 : 1 + ((e - 68) >> 1)), x = e < 34 ? e : (e < 68 ? e - 34 : ((e - 68) & 1) * 33);
        patch[y * WP32 + x] = 0.0f;
    }
    if constexpr (S3 == 0) zero_halo<LayC0, NTHR>(act, CB);                          // the halo of the flow's conv0 output layout
    else if constexpr (S3 == 2) zero_halo_q<typename SplitLays<CB>::LR0, NTHR>(act);
    else zero_halo_q<typename SplitLays<CB>::LQH, NTHR>(act);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < PPT; ++q) sum += v[q];
    const float mean = block_sum<NW>(sum, red) * (1.0f / 1024.0f);
    CNN_STAMP(17);
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < PPT; ++q) { v[q] -= mean; sq += v[q] * v[q]; }
    const float var = block_sum<NW>(sq, red + NW) * (1.0f / 1023.0f);       // torch.std: unbiased
    const float sd = sqrtf(var) + 1e-7f;
    CNN_STAMP(18);
#pragma unroll
    for (int q = 0; q < PPT; ++q) patch[((tid >> 5) + q * RPT + 1) * WP32 + (tid & 31) + 1] = v[q] / sd;
    __syncthreads();
    CNN_STAMP(1);

    // ---- one straight-line body per flow ----------------------------------------------------------------
    if constexpr (S3 == 0 && KIND == AFFNET_NET_HARDNET) {
        // Exact HardNet: conv1, conv3 and conv5 (stride 1) as Winograd F(2x2, 3x3) (cnn_mfma.h) - 4/9 of the MFMAs; each wave runs NB (tile block,
        // channel block) passes of a layer, in conv1 / conv3 two at a time on one window transform (conv3x3_wino_mfma_pair_rows).  The Winograd layers
        // load their transformed weights U from the blob (NetLayout::w_wino), ahead of their use; the first fragments of a layer are requested in front of
        // the barrier before it, where the direct-form layers (conv0, conv2, conv4) request their first weight chunk.  conv5's tensor goes to HBM for
        // the head GEMM.
        constexpr int T1M = S::T1M, T1N = S::T1N, T2M = S::T2M, T2N = S::T2N, T4M = S::T4M, T4N = S::T4N;
        constexpr int NB1 = (16 * 16 / 16) * (CB / 16) / NW, NB3 = (8 * 8 / 16) * (2 * CB / 16) / NW, NB5 = (4 * 4 / 16) * (4 * CB / 16) / NW;

        // ---- conv0: 1 -> CB, K = 9 (padded to 12), MFMA; reads `patch`, writes `act`: no barrier in between ----
        f32x4 Up[2][4];                                               // the rolling U register set of conv1 / conv3: one position row, both channel blocks of a pair
        f32x4 Uw[16];                                                 // the rolling U register set of conv5
        {
            f32x4 acc[T1M][T1N];
            conv0_mfma<NW, CB, T1M, T1N>(patch, w0, bias0, acc, wave, lane);
            CNN_STAMP(19);
            store_tiles_lds<CB, LayC0, T1M, T1N, false>(act, bias0, acc, wave, lane);
            CNN_STAMP(20);
            wino_prefetch_u_pair<NW, CB, CB, 32, NB1>(a.packed + a.off.w_wino[0], Up, wave, lane);
            __syncthreads();
        }
        if (STAMPS && a.dbg_layer == 0) { dump_planes<CB, LayC0, NTHR>(act, a.dbg_out); return; }
        CNN_STAMP(2);

        // ---- conv1: CB -> CB @32x32, Winograd -------------------------------------------------------------
        f32x4 b2[S::G2][T2N];
        f32x4 bias2[T2N];
        {
            f32x4 y[NB1][4], bw[NB1];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_wino_mfma_pair_rows<NW, CB, CB, LayC0, NB1>(act, a.packed + a.off.w_wino[0], Up, y, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(3);
            prefetch_b0<NW, 2 * CB, 16, T2M, T2N, S::G2>(a.packed + a.off.w[2], b2, wave, lane);
            prefetch_bias<NW, 16, T2M, T2N>(a.packed + a.off.b[2], bias2, wave, lane);
            wino_bias<NW, 32, CB, NB1>(a.packed + a.off.b[1], bw, wave, lane);
            __syncthreads();
            CNN_STAMP(21);
            zero_halo<LayC1, NTHR>(act, CB);
            wino_store_lds<CB, LayC1, NB1>(act, bw, y, wave, lane);
            CNN_STAMP(22);
            __syncthreads();
            CNN_STAMP(4);
        }
        if (STAMPS && a.dbg_layer == 1) { dump_planes<CB, LayC1, NTHR>(act, a.dbg_out); return; }

        // ---- conv2: CB -> 2CB, stride 2 @16x16 -----------------------------------------------------------
        {
            f32x4 acc[T2M][T2N];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma<NW, CB, 2 * CB, LayC1, 2, T2M, T2N, S::G2>(act, a.packed + a.off.w[2], b2, acc, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(5);
            wino_prefetch_u_pair<NW, 2 * CB, 2 * CB, 16, NB3>(a.packed + a.off.w_wino[1], Up, wave, lane);
            __syncthreads();
            zero_halo<LayC2, NTHR>(act, 2 * CB);
            store_tiles_lds<2 * CB, LayC2, T2M, T2N>(act, bias2, acc, wave, lane);
            __syncthreads();
            CNN_STAMP(6);
        }
        if (STAMPS && a.dbg_layer == 2) { dump_planes<2 * CB, LayC2, NTHR>(act, a.dbg_out); return; }

        // ---- conv3: 2CB -> 2CB @16x16, Winograd ----------------------------------------------------------
        f32x4 b4[S::G4][T4N];
        f32x4 bias4[T4N];
        {
            f32x4 y[NB3][4], bw[NB3];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_wino_mfma_pair_rows<NW, 2 * CB, 2 * CB, LayC2, NB3>(act, a.packed + a.off.w_wino[1], Up, y, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(7);
            prefetch_b0<NW, 4 * CB, 8, T4M, T4N, S::G4>(a.packed + a.off.w[4], b4, wave, lane);
            prefetch_bias<NW, 8, T4M, T4N>(a.packed + a.off.b[4], bias4, wave, lane);
            wino_bias<NW, 16, 2 * CB, NB3>(a.packed + a.off.b[3], bw, wave, lane);
            __syncthreads();
            zero_halo<LayC3, NTHR>(act, 2 * CB);
            wino_store_lds<2 * CB, LayC3, NB3>(act, bw, y, wave, lane);
            __syncthreads();
            CNN_STAMP(8);
        }
        if (STAMPS && a.dbg_layer == 3) { dump_planes<2 * CB, LayC3, NTHR>(act, a.dbg_out); return; }

        // ---- conv4: 2CB -> 4CB, stride 2 @8x8 --------------------------------------------------------------
        {
            f32x4 acc[T4M][T4N];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma<NW, 2 * CB, 4 * CB, LayC3, 2, T4M, T4N, S::G4>(act, a.packed + a.off.w[4], b4, acc, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(9);
            wino_prefetch_u<NW, 4 * CB, 4 * CB, 8, NB5>(a.packed + a.off.w_wino[2], Uw, wave, lane);
            __syncthreads();
            zero_halo<LayC4, NTHR>(act, 4 * CB);
            store_tiles_lds<4 * CB, LayC4, T4M, T4N>(act, bias4, acc, wave, lane);
            __syncthreads();
            CNN_STAMP(10);
        }
        if (STAMPS && a.dbg_layer == 4) { dump_planes<4 * CB, LayC4, NTHR>(act, a.dbg_out); return; }

        // ---- conv5: 4CB -> 4CB @8x8, Winograd; conv5 tensor -> HBM as [pixel][channel], the head GEMM runs over all patches ----
        f32x4 y[NB5][4], bw[NB5];
        __builtin_amdgcn_s_setprio(0);
        static_assert(NB5 == 1 && (4 * CB / 16) * 4096 <= TrunkLds<CB>::ACT, "conv5: one pass per wave, V of the layer fits the activation buffer");
        conv3x3_wino_mfma_shared_v<NW, 4 * CB, 4 * CB, LayC4>(act, a.packed + a.off.w_wino[2], Uw, y, wave, lane);
        __builtin_amdgcn_s_setprio(3);
        CNN_STAMP(11);
        wino_bias<NW, 8, 4 * CB, NB5>(a.packed + a.off.b[5], bw, wave, lane);
        if (!STAMPS || a.dbg_layer < 0) {
            wino_store_global<4 * CB, 8, NB5>(a.out + pidx * (64 * 4 * CB), bw, y, wave, lane);
            CNN_STAMP(13);
            return;
        }
        __syncthreads();
        wino_store_lds<4 * CB, LayC5, NB5>(act, bw, y, wave, lane);   // debug dump only
        __syncthreads();
        CNN_STAMP(12);
        if (STAMPS && a.dbg_layer == 5) { dump_planes<4 * CB, LayC5, NTHR>(act, a.dbg_out); return; }
    } else if constexpr (S3 == 0) {
        // Exact AffNet / OriNet.  OriNet: conv1, conv3 and conv5 (stride 1) as Winograd F(2x2, 3x3), one row of four transform positions at a time
        // (conv3x3_wino_mfma_rows: the 128-register budget of two workgroups per CU) - 4/9 of their MFMAs; U = G g G^T comes from a.wino_u, which
        // wino_derive_u_kernel fills from the blob's taps in front of every launch.  AffNet keeps conv1 .. conv5 in the direct form: its output decides the
        // shape filter, whose eigenvalue test (shape_filter.h: d1 = tr^2 - 4 det > 0) turns on the LAST bits of A for near-isotropic shapes, so any other
        // rounding changes which keypoints a call returns (measured: 124 of 128 000 ids at the headline configuration).  conv0, conv2, conv4 (and AffNet's conv5) in
        // the direct form for both; conv5 straight into the heads (AffNet from the direct form's accumulators, OriNet from its Winograd fragments).
        constexpr int T1M = S::T1M, T1N = S::T1N, T2M = S::T2M, T2N = S::T2N, T4M = S::T4M, T4N = S::T4N;
        static_assert(NW == 8 && CB == 16, "Wino16 describes the 16-channel trunks on 8 waves");
        f32x4 b4[S::G4][T4N];
        f32x4 bias4[T4N];
        if constexpr (KIND == AFFNET_NET_ORINET) {
            constexpr int NB1 = Wino16::NB1, NB3 = Wino16::NB3;
            // ---- conv0: 1 -> CB, K = 9 (padded to 12), MFMA; reads `patch`, writes `act`: no barrier in between ----
            {
                f32x4 acc[T1M][T1N];
                conv0_mfma<NW, CB, T1M, T1N>(patch, w0, bias0, acc, wave, lane);
                CNN_STAMP(19);
                store_tiles_lds<CB, LayC0, T1M, T1N, false>(act, bias0, acc, wave, lane);
                CNN_STAMP(20);
                __syncthreads();
            }
            if (STAMPS && a.dbg_layer == 0) { dump_planes<CB, LayC0, NTHR>(act, a.dbg_out); return; }
            CNN_STAMP(2);

            // ---- conv1: CB -> CB @32x32, Winograd ------------------------------------------------------------
            f32x4 b2[S::G2][T2N];
            f32x4 bias2[T2N];
            {
                f32x4 y[NB1][4], bw[NB1];
                conv3x3_wino_mfma_rows<NW, CB, CB, LayC0, NB1>(act, a.wino_u, Ur, y, wave, lane);
                CNN_STAMP(3);
                prefetch_b0<NW, 2 * CB, 16, T2M, T2N, S::G2>(a.packed + a.off.w[2], b2, wave, lane);
                prefetch_bias<NW, 16, T2M, T2N>(a.packed + a.off.b[2], bias2, wave, lane);
                wino_bias<NW, 32, CB, NB1>(a.packed + a.off.b[1], bw, wave, lane);
                __syncthreads();
                CNN_STAMP(21);
                zero_halo<LayC1, NTHR>(act, CB);
                wino_store_lds<CB, LayC1, NB1>(act, bw, y, wave, lane);
                CNN_STAMP(22);
                __syncthreads();
                CNN_STAMP(4);
            }
            if (STAMPS && a.dbg_layer == 1) { dump_planes<CB, LayC1, NTHR>(act, a.dbg_out); return; }

            // ---- conv2: CB -> 2CB, stride 2 @16x16 -----------------------------------------------------------
            {
                f32x4 acc[T2M][T2N];
                conv3x3_mfma<NW, CB, 2 * CB, LayC1, 2, T2M, T2N, S::G2>(act, a.packed + a.off.w[2], b2, acc, wave, lane);
                CNN_STAMP(5);
                wino_prefetch_u_row<NW, 2 * CB, 2 * CB, 16, NB3>(a.wino_u + Wino16::offset(3), Ur, wave, lane);
                __syncthreads();
                zero_halo<LayC2, NTHR>(act, 2 * CB);
                store_tiles_lds<2 * CB, LayC2, T2M, T2N>(act, bias2, acc, wave, lane);
                __syncthreads();
                CNN_STAMP(6);
            }
            if (STAMPS && a.dbg_layer == 2) { dump_planes<2 * CB, LayC2, NTHR>(act, a.dbg_out); return; }

            // ---- conv3: 2CB -> 2CB @16x16, Winograd ----------------------------------------------------------
            {
                f32x4 y[NB3][4], bw[NB3];
                conv3x3_wino_mfma_rows<NW, 2 * CB, 2 * CB, LayC2, NB3>(act, a.wino_u + Wino16::offset(3), Ur, y, wave, lane);
                CNN_STAMP(7);
                prefetch_b0<NW, 4 * CB, 8, T4M, T4N, S::G4>(a.packed + a.off.w[4], b4, wave, lane);
                prefetch_bias<NW, 8, T4M, T4N>(a.packed + a.off.b[4], bias4, wave, lane);
                wino_bias<NW, 16, 2 * CB, NB3>(a.packed + a.off.b[3], bw, wave, lane);
                __syncthreads();
                zero_halo<LayC3, NTHR>(act, 2 * CB);
                wino_store_lds<2 * CB, LayC3, NB3>(act, bw, y, wave, lane);
                __syncthreads();
                CNN_STAMP(8);
            }
            if (STAMPS && a.dbg_layer == 3) { dump_planes<2 * CB, LayC3, NTHR>(act, a.dbg_out); return; }

        } else {
            static_assert(T1M * 8 > S::AREG, "conv1: two A sets of T1M float4 do not fit -> rolling single set (conv3x3_mfma_roll)");
            // ---- conv0: 1 -> CB, K = 9 (padded to 12), MFMA; reads `patch`, writes `act`: no barrier in between ----
            f32x4 bias1[T1N];
            {
                f32x4 acc[T1M][T1N];
                conv0_mfma<NW, CB, T1M, T1N>(patch, w0, bias0, acc, wave, lane);
                CNN_STAMP(19);
                prefetch_bias<NW, 32, T1M, T1N>(a.packed + a.off.b[1], bias1, wave, lane);
                store_tiles_lds<CB, LayC0, T1M, T1N, false>(act, bias0, acc, wave, lane);
                CNN_STAMP(20);
                __syncthreads();
            }
            if (STAMPS && a.dbg_layer == 0) { dump_planes<CB, LayC0, NTHR>(act, a.dbg_out); return; }
            CNN_STAMP(2);

            // ---- conv1: CB -> CB @32x32 --------------------------------------------------------------------
            f32x4 b2[S::G2][T2N];
            f32x4 bias2[T2N];
            {
                f32x4 acc[T1M][T1N];
                conv3x3_mfma_roll<NW, CB, CB, LayC0, 1, T1M, T1N>(act, a.packed + a.off.w[1], b1, acc, wave, lane);
                CNN_STAMP(3);
                prefetch_b0<NW, 2 * CB, 16, T2M, T2N, S::G2>(a.packed + a.off.w[2], b2, wave, lane);
                prefetch_bias<NW, 16, T2M, T2N>(a.packed + a.off.b[2], bias2, wave, lane);
                __syncthreads();
                CNN_STAMP(21);
                zero_halo<LayC1, NTHR>(act, CB);
                store_tiles_lds<CB, LayC1, T1M, T1N>(act, bias1, acc, wave, lane);
                CNN_STAMP(22);
                __syncthreads();
                CNN_STAMP(4);
            }
            if (STAMPS && a.dbg_layer == 1) { dump_planes<CB, LayC1, NTHR>(act, a.dbg_out); return; }

            // ---- conv2: CB -> 2CB, stride 2 @16x16 -----------------------------------------------------------
            f32x4 b3[S::G3][T2N];
            f32x4 bias3[T2N];
            {
                f32x4 acc[T2M][T2N];
                conv3x3_mfma<NW, CB, 2 * CB, LayC1, 2, T2M, T2N, S::G2>(act, a.packed + a.off.w[2], b2, acc, wave, lane);
                CNN_STAMP(5);
                prefetch_b0<NW, 2 * CB, 16, T2M, T2N, S::G3>(a.packed + a.off.w[3], b3, wave, lane);
                prefetch_bias<NW, 16, T2M, T2N>(a.packed + a.off.b[3], bias3, wave, lane);
                __syncthreads();
                zero_halo<LayC2, NTHR>(act, 2 * CB);
                store_tiles_lds<2 * CB, LayC2, T2M, T2N>(act, bias2, acc, wave, lane);
                __syncthreads();
                CNN_STAMP(6);
            }
            if (STAMPS && a.dbg_layer == 2) { dump_planes<2 * CB, LayC2, NTHR>(act, a.dbg_out); return; }

            // ---- conv3: 2CB -> 2CB @16x16 --------------------------------------------------------------------
            {
                f32x4 acc[T2M][T2N];
                conv3x3_mfma<NW, 2 * CB, 2 * CB, LayC2, 1, T2M, T2N, S::G3>(act, a.packed + a.off.w[3], b3, acc, wave, lane);
                CNN_STAMP(7);
                prefetch_b0<NW, 4 * CB, 8, T4M, T4N, S::G4>(a.packed + a.off.w[4], b4, wave, lane);
                prefetch_bias<NW, 8, T4M, T4N>(a.packed + a.off.b[4], bias4, wave, lane);
                __syncthreads();
                zero_halo<LayC3, NTHR>(act, 2 * CB);
                store_tiles_lds<2 * CB, LayC3, T2M, T2N>(act, bias3, acc, wave, lane);
                __syncthreads();
                CNN_STAMP(8);
            }
            if (STAMPS && a.dbg_layer == 3) { dump_planes<2 * CB, LayC3, NTHR>(act, a.dbg_out); return; }

        }

        // ---- conv4: 2CB -> 4CB, stride 2 @8x8 --------------------------------------------------------------
        f32x4 b5[S::G5][T4N];
        f32x4 bias5[T4N];
        {
            f32x4 acc[T4M][T4N];
            conv3x3_mfma<NW, 2 * CB, 4 * CB, LayC3, 2, T4M, T4N, S::G4>(act, a.packed + a.off.w[4], b4, acc, wave, lane);
            CNN_STAMP(9);
            if constexpr (KIND == AFFNET_NET_ORINET) {
                wino5_prefetch_u(a.wino_u + Wino16::offset(5), Ur, wave, lane);
            } else {
                prefetch_b0<NW, 4 * CB, 8, T4M, T4N, S::G5>(a.packed + a.off.w[5], b5, wave, lane);
                prefetch_bias<NW, 8, T4M, T4N>(a.packed + a.off.b[5], bias5, wave, lane);
            }
            __syncthreads();
            zero_halo<LayC4, NTHR>(act, 4 * CB);
            store_tiles_lds<4 * CB, LayC4, T4M, T4N>(act, bias4, acc, wave, lane);
            __syncthreads();
            CNN_STAMP(10);
        }
        if (STAMPS && a.dbg_layer == 4) { dump_planes<4 * CB, LayC4, NTHR>(act, a.dbg_out); return; }

        if constexpr (KIND == AFFNET_NET_ORINET) {
            // ---- conv5: 4CB -> 4CB @8x8, Winograd, a wave pair per channel block (conv3x3_wino_mfma_half_rows, wino5_combine); its 2 x 2-pixel fragments go
            // into the head's 10 x 10 copy (over conv4's output, which is dead by then), then the head's per-wave partial sums ----
            static_assert(Wino5::X >= 16 * LayC4::PSG && Wino5::X + Wino5::X_FLOATS <= TrunkLds<CB>::TOTAL && Wino5::HEAD + 100 * ORI_HP <= Wino5::X,
                          "conv5: the exchange lies behind conv4's output inside the LDS array, the head copy in front of the exchange");
            f32x4 acc[2][4], y[2], hw[2][T4M];
            conv3x3_wino_mfma_half_rows<NW, LayC4>(act, a.wino_u + Wino16::offset(5), Ur, acc, wave, lane);
            CNN_STAMP(11);
            const f32x4 bw = *reinterpret_cast<const f32x4*>(&a.packed[a.off.b[5] + (wave >> 1) * 16 + 4 * (lane >> 4)]);
            const OriHeadLane HL = OriHeadLane::of<T4M>(wave, lane);
            if (!STAMPS || a.dbg_layer < 0) ori_head_weights<T4M>(a.packed + a.off.head_w, HL, hw);
            wino5_combine(lds, acc, y, wave, lane);
            if (!STAMPS || a.dbg_layer < 0) {
                float* copy = lds + Wino5::HEAD;
                ori_head_zero_halo<NTHR>(copy, tid);
                wino5_store_lds<10, ORI_HP, 4>(copy + 11 * ORI_HP, bw, y, wave, lane);
                int pbase[T4M];
                ori_head_pbase<T4M>(HL, pbase);
                ori_head_reduce<T4M>(hw, pbase, a.out + pidx * HEAD_PART_ORI, copy, wave, lane);
                CNN_STAMP(13);
                return;
            }
            __syncthreads();
            wino5_store_lds<LayC5::WP, 4, LayC5::PSG>(act + (LayC5::WP + 1) * 4, bw, y, wave, lane);   // debug dump only
            __syncthreads();
            CNN_STAMP(12);
            if (STAMPS && a.dbg_layer == 5) { dump_planes<4 * CB, LayC5, NTHR>(act, a.dbg_out); return; }
            return;
        }
        // ---- conv5: 4CB -> 4CB @8x8, then the head's per-wave partial sums ---------------------------------
        f32x4 acc[T4M][T4N];
        conv3x3_mfma<NW, 4 * CB, 4 * CB, LayC4, 1, T4M, T4N, S::G5>(act, a.packed + a.off.w[5], b5, acc, wave, lane);
        CNN_STAMP(11);
        if (!STAMPS || a.dbg_layer < 0) {
            head_partials<T4M>(a.packed + a.off.head_w, bias5, acc, a.out + pidx * HEAD_PART_AFF, wave, lane);
            CNN_STAMP(13);
            return;
        }
        __syncthreads();
        store_tiles_lds<4 * CB, LayC5, T4M, T4N>(act, bias5, acc, wave, lane);   // debug dump only
        __syncthreads();
        CNN_STAMP(12);
        if (STAMPS && a.dbg_layer == 5) { dump_planes<4 * CB, LayC5, NTHR>(act, a.dbg_out); return; }
    } else if constexpr (KIND == AFFNET_NET_HARDNET) {
        // Split HardNet.  AFFNET_ARITH_FP32_SPLIT3 (affnet_set_arith): conv1 .. conv5 on split operands - every fp32 operand as three bf16 terms, six
        // v_mfma_f32_16x16x32_bf16 per product, fp32 accumulate (SPLIT2H: two fp16 terms).  conv0 .. conv4 write their outputs PRE-SPLIT (SplitLays, LayQ / LayR),
        // conv1 .. conv5 read ready fragments (conv3x3_mfma_s3q): no VALU work inside the MFMA loops ("Split-operand trunks").
        // The first weight fragments of a loop are requested before the barriers / epilogue in front of it.
        // One workgroup per CU: optionally (affnet_debug_split3_variant bit 0) the two waves of a SIMD take turns at the higher priority
        // inside the loops.  Round 3's tile-major loops gained 2.5 % from it; with the term-major loops it costs 1 % (default off).
        using SL = SplitLays<CB>;
        using LQH = typename SL::LQH;
        using LQH2 = typename SL::LQH2;
        using LR0 = typename SL::LR0;
        using LR1 = typename SL::LR1;
        constexpr int TERMS = S3;
        constexpr bool WHOLE = TERMS == 2;
        f32x4 bias1[2];
        const int s3_alt = a.s3_alt;                                        // variant bits for the loops (conv3x3_mfma_s3q)
        // conv2 / conv3 outputs, 64 channels @16x16 (122 KB / 90 KB): read at stride 1 (conv3) and, conv3's output written in place, at stride 2 (conv4).  No group
        // stride serves both readers (tools/lds_bank_model.py): GS = 0 (mod 256) leaves conv4's two-row reader with 2-way conflicts, GS = 16 conv3's one-row reader.
        // LayR takes conv4's here: its 4 x 1 tiles are the more LDS-bound (probe: -1350 cycles for conv4, +300 for conv3's 4 x 2); a second layout for conv3's
        // output with the other stride cost 0.8 k cycles per patch for zeroing its halo again (measured)
        using LQ2 = std::conditional_t<TERMS == 2, LayR<16, 16, 20, 2 * CB, 16>, LayQ<16, 16, 18, 2 * CB, 0, 3>>;
        using LQ4 = std::conditional_t<TERMS == 2, LayR<8, 8, 12, 4 * CB, 0>, LayQ<8, 8, 16, 4 * CB, 128, 3>>;        // conv4 output: 128 channels @8x8 (122 KB / 60 KB)
        static_assert(LQ2::BYTES <= TrunkLds<CB>::ACT * 4 && LQ4::BYTES <= TrunkLds<CB>::ACT * 4, "pre-split layouts must fit the activation buffer");
        char* base = reinterpret_cast<char*>(act);
        // three terms: conv0 + conv1 in two half-patch passes - the pre-split conv0 output of 32 channels @32x32 would be 222 KB, half of it (16 rows +
        // a halo row either side) is 115 KB; two terms (WHOLE): 145 KB, conv0 runs once and the two half loops of conv1 / conv2 read 16-row views
        f32x4 acc_a[4][2], acc_b[4][2];
        // register blockings per layer from tools/probes/s3_loop_probe (profiles/r04_s3_s3_loop_probe_tilings.txt): conv1 / conv3 4 pixel tiles x 2 channel
        // tiles per wave; conv2 / conv4 / conv5 4 x 1 (one weight fragment feeds four pixel tiles: 85.0 / 86.0 / 89.0 % of the pipe floor vs 78.5 / 83.8 /
        // 87.0 % for 2 x 2)
        S3W<2> wf1;
        S3W<1> wf2;
        f32x4 acc2_a[4][1], acc2_b[4][1], bias2[1];
        f32x4 acc2w[4][2], bias2w[2];                                    // (two-term flow: conv2 as one 4 x 2 loop)
        if constexpr (WHOLE) {
            // two terms: conv0 once, then conv1 as ONE loop over the whole patch (8 pixel tiles x 2 channel tiles per wave: the weights stream once, not once per half)
            // and conv2 as one 4 x 2 loop
            f32x4 acc1[8][2];
            S3W<2> wf2w;
            s3_prefetch_w0<NW, CB, CB, 64, 8, 2, TERMS>(a.packed + a.off.w_s3[1], wf1, wave, lane);
            prefetch_bias<NW, 32, 8, 2>(a.packed + a.off.b[1], bias1, wave, lane);
            conv0_whole_split_q<NW, LR0, 2>(patch, w0, bias0, act, wave, lane);
            __syncthreads();
            CNN_STAMP(2);
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma_s3q<NW, CB, CB, LR0, 1, 8, 2>(act, a.packed + a.off.w_s3[1], wf1, acc1, wave, lane, s3_alt);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(3);
            s3_prefetch_w0<NW, CB, 2 * CB, 16, 4, 2, TERMS>(a.packed + a.off.w_s3[2], wf2w, wave, lane);
            prefetch_bias<NW, 16, 4, 2>(a.packed + a.off.b[2], bias2w, wave, lane);
            __syncthreads();
            zero_halo_q<LR1, NTHR>(act);                                 // another group stride than LR0 (the stride-2 reader's): the halo cells move
            store_tiles_split_q<CB, LR1, 8, 2>(act, bias1, acc1, wave, lane);
            __syncthreads();
            CNN_STAMP(4);
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma_s3q<NW, CB, 2 * CB, LR1, 2, 4, 2>(act, a.packed + a.off.w_s3[2], wf2w, acc2w, wave, lane, s3_alt);
            __builtin_amdgcn_s_setprio(3);
        } else {
            s3_prefetch_w0<NW, CB, CB, 32, 4, 2, TERMS>(a.packed + a.off.w_s3[1], wf1, wave, lane);
            prefetch_bias<NW, 32, 8, 2>(a.packed + a.off.b[1], bias1, wave, lane);
            conv0_half_split_q<NW, LQH, 2>(patch, w0, bias0, act, 0, wave, lane);
            __syncthreads();
            CNN_STAMP(2);
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma_s3q<NW, CB, CB, LQH, 1, 4, 2>(act, a.packed + a.off.w_s3[1], wf1, acc_a, wave, lane, s3_alt);
            __builtin_amdgcn_s_setprio(3);
            __syncthreads();
            if (tid < LQH::SLOTS * 4 * 32) {                             // pass 0 left conv0 row 16 in the bottom halo row: zero again (slots x 4 groups x 32 cells)
                const int t = tid / 128, g = (tid >> 5) & 3, x = tid & 31;
                *reinterpret_cast<f32x4*>(base + g * LQH::GS + LQH::at(17, x + 1) + t * LQH::TSTEP) = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            conv0_half_split_q<NW, LQH, 2>(patch, w0, bias0, act, 1, wave, lane);
            __syncthreads();
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma_s3q<NW, CB, CB, LQH, 1, 4, 2>(act, a.packed + a.off.w_s3[1], wf1, acc_b, wave, lane, s3_alt);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(3);
            s3_prefetch_w0<NW, CB, 2 * CB, 8, 4, 1, TERMS>(a.packed + a.off.w_s3[2], wf2, wave, lane);
            bias2[0] = *reinterpret_cast<const f32x4*>(&a.packed[a.off.b[2] + (wave >> 1) * 16 + 4 * (lane >> 4)]);      // MG = 8 tiles / 4 = 2: channel tile = wave / 2
            __syncthreads();
            // conv1's output goes back into the same half layout, pre-split, and conv2 (stride 2: output rows 0 .. 7 read input rows
            // -1 .. 15, rows 8 .. 15 read 15 .. 31) runs in two passes as well
            zero_halo_q<LQH2, NTHR>(act);                                // another group stride than LQH (bank conflicts of the stride-2 reader)
            store_tiles_split_q<CB, LQH2, 4, 2>(act, bias1, acc_a, wave, lane);
            __syncthreads();
            CNN_STAMP(4);
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma_s3q<NW, CB, 2 * CB, LQH2, 2, 4, 1>(act, a.packed + a.off.w_s3[2], wf2, acc2_a, wave, lane, s3_alt);
            __builtin_amdgcn_s_setprio(3);
            __syncthreads();
            store_tiles_split_q<CB, LQH2, 4, 2>(act, bias1, acc_b, wave, lane);
            if (wave == 7) {                                             // conv1 row 15 (tiles 2, 3 of wave 7 in pass 0) = the top halo row of pass 1
                const int n = lane & 15;
#pragma unroll
                for (int i = 2; i < 4; ++i) split_store_tile_q<LQH2, 2>(base, LQH2::at(0, (i - 2) * 16 + n + 1), 0, bias1, acc_a[i], lane >> 4);
            }
            __syncthreads();
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma_s3q<NW, CB, 2 * CB, LQH2, 2, 4, 1>(act, a.packed + a.off.w_s3[2], wf2, acc2_b, wave, lane, s3_alt);
            __builtin_amdgcn_s_setprio(3);
        }
        CNN_STAMP(5);
        S3W<2> wf3;
        S3W<1> wf4, wf5;
        f32x4 bias3[2], bias4[1], bias5s[1];
        s3_prefetch_w0<NW, 2 * CB, 2 * CB, 16, 4, 2, TERMS>(a.packed + a.off.w_s3[3], wf3, wave, lane);
        prefetch_bias<NW, 16, 4, 2>(a.packed + a.off.b[3], bias3, wave, lane);
        __syncthreads();
        zero_halo_q<LQ2, NTHR>(act);
        if constexpr (WHOLE) store_tiles_split_q<2 * CB, LQ2, 4, 2>(act, bias2w, acc2w, wave, lane);
        else {
            store_tiles_split_q<2 * CB, LQ2, 4, 1, 8>(act, bias2, acc2_a, wave, lane, 0);
            store_tiles_split_q<2 * CB, LQ2, 4, 1, 8>(act, bias2, acc2_b, wave, lane, 8);
        }
        __syncthreads();
        CNN_STAMP(6);
        {
            f32x4 acc_[4][2];                                            // conv3: 64 -> 64 @16x16
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma_s3q<NW, 2 * CB, 2 * CB, LQ2, 1, 4, 2>(act, a.packed + a.off.w_s3[3], wf3, acc_, wave, lane, s3_alt);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(7);
            s3_prefetch_w0<NW, 2 * CB, 4 * CB, 4, 4, 1, TERMS>(a.packed + a.off.w_s3[4], wf4, wave, lane);
            prefetch_bias<NW, 8, 4, 1>(a.packed + a.off.b[4], bias4, wave, lane);
            __syncthreads();
            store_tiles_split_q<2 * CB, LQ2, 4, 2>(act, bias3, acc_, wave, lane);      // same layout in place: the halo is still zero
            __syncthreads();
            CNN_STAMP(8);
        }
        {
            f32x4 acc_[4][1];                                            // conv4: 64 -> 128, stride 2 -> 8x8
            __builtin_amdgcn_s_setprio(0);
            conv3x3_mfma_s3q<NW, 2 * CB, 4 * CB, LQ2, 2, 4, 1>(act, a.packed + a.off.w_s3[4], wf4, acc_, wave, lane, s3_alt);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(9);
            s3_prefetch_w0<NW, 4 * CB, 4 * CB, 4, 4, 1, TERMS>(a.packed + a.off.w_s3[5], wf5, wave, lane);
            prefetch_bias<NW, 8, 4, 1>(a.packed + a.off.b[5], bias5s, wave, lane);
            __syncthreads();
            zero_halo_q<LQ4, NTHR>(act);
            store_tiles_split_q<4 * CB, LQ4, 4, 1>(act, bias4, acc_, wave, lane);
            __syncthreads();
            CNN_STAMP(10);
        }
        f32x4 acc5[4][1];                                                // conv5: 128 -> 128 @8x8, conv5 tensor -> HBM for the head GEMM
        __builtin_amdgcn_s_setprio(0);
        conv3x3_mfma_s3q<NW, 4 * CB, 4 * CB, LQ4, 1, 4, 1>(act, a.packed + a.off.w_s3[5], wf5, acc5, wave, lane, s3_alt);
        __builtin_amdgcn_s_setprio(3);
        CNN_STAMP(11);
        store_tiles_global<4 * CB, 4, 1>(a.out + pidx * (64 * 4 * CB), bias5s, acc5, wave, lane);
    } else {
        // Split AffNet / OriNet, same structure as split HardNet: conv0 .. conv2 in two half-patch passes on pre-split layouts (conv1 / conv2 have
        // 16 input channels: two taps per k = 32 step), conv3 .. conv5 whole.
        // (tried in round 4: the phases outside the MFMA loops at a higher issue priority than the loops - with two workgroups per CU a young
        // workgroup crawls through input / conv0 / epilogues next to an older one in its loops, conv0 of half a patch takes 9 - 10 k cycles for
        // ~150 instructions per wave.  Zero-sum as in the exact path: 4.12 vs 4.10 - 4.13 ms per 48000 patches.  Removed.)
        constexpr int T4M = S::T4M, T4N = S::T4N;
        using SL = SplitLays<CB>;
        using LQH = typename SL::LQH;
        using LQH2 = typename SL::LQH2;
        using LR0 = typename SL::LR0;
        using LR0H = typename SL::LR0H;
        using LR1 = typename SL::LR1;
        using LR1H = typename SL::LR1H;
        constexpr int TERMS = S3;
        constexpr bool WHOLE = TERMS == 2;
        f32x4 bias1[1];
        // conv2 / conv3 outputs: 32 channels @16x16 (61 KB / 45 KB).  LayR: GS = 0 (mod 256) here - with two workgroups per CU conv3's one-row reader is LDS-bound and
        // the 2-way conflicts of the HardNet branch's choice cost it 10 % (probe: 7.1 k vs 6.5 k cycles), while conv4 (2 x 1 tiles) is the same with or without its own
        using LQ2 = std::conditional_t<TERMS == 2, LayR<16, 16, 20, 2 * CB, 0>, LayQ<16, 16, 18, 2 * CB, 0, 3>>;
        using LQ4 = std::conditional_t<TERMS == 2, LayR<8, 8, 12, 4 * CB, 0>, LayQ<8, 8, 16, 4 * CB, 128, 3>>;        // conv4 output: 64 channels @8x8 (61 KB / 30 KB)
        static_assert(LQ2::BYTES <= TrunkLds<CB>::ACT * 4 && LQ4::BYTES <= TrunkLds<CB>::ACT * 4, "pre-split layouts must fit the activation buffer");
        char* base = reinterpret_cast<char*>(act);
        f32x4 acc_a[4][1], acc_b[4][1];
        // (128 VGPRs at two workgroups per CU: a loop's first weight fragments are requested right in front of it here - held across the
        // previous epilogue like in the HardNet branch they cost 17 / 23 spilled registers)
        S3W<1> wf1, wf2;
        f32x4 acc2_a[2][1], acc2_b[2][1], bias2[1];
        if constexpr (WHOLE) {
            prefetch_bias_fresh<NW, 32, 8, 1>(a.packed + a.off.b[1], bias1, wave, lane);
            conv0_whole_split_q<NW, LR0, 1>(patch, w0, bias0, act, wave, lane);
            s3_prefetch_w0<NW, CB, CB, 32, 4, 1, TERMS>(a.packed + a.off.w_s3[1], wf1, wave, lane);
            __syncthreads();
            CNN_STAMP(2);
            conv3x3_mfma_s3q<NW, CB, CB, LR0H, 1, 4, 1>(act, a.packed + a.off.w_s3[1], wf1, acc_a, wave, lane, false);
            conv3x3_mfma_s3q<NW, CB, CB, LR0H, 1, 4, 1>(act + LR0::at(16, 0) / 4, a.packed + a.off.w_s3[1], wf1, acc_b, wave, lane, false);
            CNN_STAMP(3);
            {
                int l2 = lane;
                asm volatile("" : "+v"(l2));
                bias2[0] = *reinterpret_cast<const f32x4*>(&a.packed[a.off.b[2] + (wave >> 2) * 16 + 4 * (l2 >> 4)]);
            }
            __syncthreads();
            zero_halo_q<LR1, NTHR>(act);                                     // another group stride than LR0 (the stride-2 reader's): the halo cells move
            store_tiles_split_q<CB, LR1, 4, 1, 16>(act, bias1, acc_a, wave, lane, 0);
            store_tiles_split_q<CB, LR1, 4, 1, 16>(act, bias1, acc_b, wave, lane, 16);
            s3_prefetch_w0<NW, CB, 2 * CB, 8, 2, 1, TERMS>(a.packed + a.off.w_s3[2], wf2, wave, lane);
            __syncthreads();
            CNN_STAMP(4);
            conv3x3_mfma_s3q<NW, CB, 2 * CB, LR1H, 2, 2, 1>(act, a.packed + a.off.w_s3[2], wf2, acc2_a, wave, lane, false);
            conv3x3_mfma_s3q<NW, CB, 2 * CB, LR1H, 2, 2, 1>(act + LR1::at(16, 0) / 4, a.packed + a.off.w_s3[2], wf2, acc2_b, wave, lane, false);
        } else {
            prefetch_bias_fresh<NW, 32, 8, 1>(a.packed + a.off.b[1], bias1, wave, lane);
            conv0_half_split_q<NW, LQH, 1>(patch, w0, bias0, act, 0, wave, lane);
            s3_prefetch_w0<NW, CB, CB, 32, 4, 1, TERMS>(a.packed + a.off.w_s3[1], wf1, wave, lane);
            __syncthreads();
            CNN_STAMP(2);
            conv3x3_mfma_s3q<NW, CB, CB, LQH, 1, 4, 1>(act, a.packed + a.off.w_s3[1], wf1, acc_a, wave, lane, false);
            __syncthreads();
            if (tid < LQH::SLOTS * 2 * 32) {                                 // pass 0 left conv0 row 16 in the bottom halo row: zero again (slots x 2 groups x 32 cells)
                const int t = tid >> 6, g = (tid >> 5) & 1, x = tid & 31;
                *reinterpret_cast<f32x4*>(base + g * LQH::GS + LQH::at(17, x + 1) + t * LQH::TSTEP) = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            conv0_half_split_q<NW, LQH, 1>(patch, w0, bias0, act, 1, wave, lane);
            s3_prefetch_w0<NW, CB, CB, 32, 4, 1, TERMS>(a.packed + a.off.w_s3[1], wf1, wave, lane);
            __syncthreads();
            conv3x3_mfma_s3q<NW, CB, CB, LQH, 1, 4, 1>(act, a.packed + a.off.w_s3[1], wf1, acc_b, wave, lane, false);
            CNN_STAMP(3);
            {
                int l2 = lane;
                asm volatile("" : "+v"(l2));
                bias2[0] = *reinterpret_cast<const f32x4*>(&a.packed[a.off.b[2] + (wave >> 2) * 16 + 4 * (l2 >> 4)]);
            }
            __syncthreads();
            zero_halo_q<LQH2, NTHR>(act);                                    // another group stride than LQH (bank conflicts of the stride-2 reader)
            store_tiles_split_q<CB, LQH2, 4, 1>(act, bias1, acc_a, wave, lane);
            s3_prefetch_w0<NW, CB, 2 * CB, 8, 2, 1, TERMS>(a.packed + a.off.w_s3[2], wf2, wave, lane);
            __syncthreads();
            CNN_STAMP(4);
            conv3x3_mfma_s3q<NW, CB, 2 * CB, LQH2, 2, 2, 1>(act, a.packed + a.off.w_s3[2], wf2, acc2_a, wave, lane, false);
            __syncthreads();
            store_tiles_split_q<CB, LQH2, 4, 1>(act, bias1, acc_b, wave, lane);
            if (wave == 7) {                                                 // conv1 row 15 (tiles 2, 3 of wave 7 in pass 0) = the top halo row of pass 1
                const int n = lane & 15;
#pragma unroll
                for (int i = 2; i < 4; ++i) split_store_tile_q<LQH2, 1>(base, LQH2::at(0, (i - 2) * 16 + n + 1), 0, bias1, acc_a[i], lane >> 4);
            }
            s3_prefetch_w0<NW, CB, 2 * CB, 8, 2, 1, TERMS>(a.packed + a.off.w_s3[2], wf2, wave, lane);
            __syncthreads();
            conv3x3_mfma_s3q<NW, CB, 2 * CB, LQH2, 2, 2, 1>(act, a.packed + a.off.w_s3[2], wf2, acc2_b, wave, lane, false);
        }
        CNN_STAMP(5);
        // conv3 / conv4: four / two pixel tiles x ONE channel tile per wave (probe: conv3 64.8 % of the pipe floor vs 58.2 % for 2 x 2, conv4 60.6 % vs
        // 39.4 % for 1 x 2 - a weight fragment that feeds a single pixel tile leaves the loop waiting on L2)
        S3W<1> wf3, wf4;
        f32x4 bias3[1], bias4[1];
        __syncthreads();
        zero_halo_q<LQ2, NTHR>(act);
        store_tiles_split_q<2 * CB, LQ2, 2, 1, 8>(act, bias2, acc2_a, wave, lane, 0);
        store_tiles_split_q<2 * CB, LQ2, 2, 1, 8>(act, bias2, acc2_b, wave, lane, 8);
        s3_prefetch_w0<NW, 2 * CB, 2 * CB, 16, 4, 1, TERMS>(a.packed + a.off.w_s3[3], wf3, wave, lane);
        prefetch_bias_fresh<NW, 16, 4, 1>(a.packed + a.off.b[3], bias3, wave, lane);
        __syncthreads();
        CNN_STAMP(6);
        {
            f32x4 acc_[4][1];                                            // conv3: 32 -> 32 @16x16
            conv3x3_mfma_s3q<NW, 2 * CB, 2 * CB, LQ2, 1, 4, 1>(act, a.packed + a.off.w_s3[3], wf3, acc_, wave, lane, false);
            CNN_STAMP(7);
            __syncthreads();
            store_tiles_split_q<2 * CB, LQ2, 4, 1>(act, bias3, acc_, wave, lane);      // in place: the halo is still zero
            s3_prefetch_w0<NW, 2 * CB, 4 * CB, 4, 2, 1, TERMS>(a.packed + a.off.w_s3[4], wf4, wave, lane);
            prefetch_bias_fresh<NW, 8, 2, 1>(a.packed + a.off.b[4], bias4, wave, lane);
            __syncthreads();
            CNN_STAMP(8);
        }
        S3W<T4N> wf5;
        f32x4 bias5s[T4N];
        {
            f32x4 acc_[2][1];                                            // conv4: 32 -> 64, stride 2 -> 8x8
            conv3x3_mfma_s3q<NW, 2 * CB, 4 * CB, LQ2, 2, 2, 1>(act, a.packed + a.off.w_s3[4], wf4, acc_, wave, lane, false);
            CNN_STAMP(9);
            __syncthreads();
            zero_halo_q<LQ4, NTHR>(act);
            store_tiles_split_q<4 * CB, LQ4, 2, 1>(act, bias4, acc_, wave, lane);
            s3_prefetch_w0<NW, 4 * CB, 4 * CB, 4, T4M, T4N, TERMS>(a.packed + a.off.w_s3[5], wf5, wave, lane);
            prefetch_bias_fresh<NW, 8, T4M, T4N>(a.packed + a.off.b[5], bias5s, wave, lane);
            __syncthreads();
            CNN_STAMP(10);
        }
        f32x4 acc5[T4M][T4N];                                            // conv5: 64 -> 64 @8x8 in the exact path's tiling (the heads read it)
        conv3x3_mfma_s3q<NW, 4 * CB, 4 * CB, LQ4, 1, T4M, T4N>(act, a.packed + a.off.w_s3[5], wf5, acc5, wave, lane, false);
        CNN_STAMP(11);
        int lane_h = lane;                                               // opaque: 4 * (lane >> 4) is recomputed here, not carried (and spilled) from the kernel's top
        asm volatile("" : "+v"(lane_h));
        if constexpr (KIND == AFFNET_NET_ORINET)
            head_partials_ori_lds<T4M, NTHR>(a.packed + a.off.head_w, bias5s, acc5, a.out + pidx * HEAD_PART_ORI, act, wave, lane_h, tid);
        else
            head_partials<T4M>(a.packed + a.off.head_w, bias5s, acc5, a.out + pidx * HEAD_PART_AFF, wave, lane_h);
        CNN_STAMP(13);
    }
}

// ---- AffNet / OriNet heads, second half: combine the eight per-wave partials of a patch ---------------------------------
//   AffNet : + bias -> tanh -> [[1+x0, 0],[x1, 1+x2]] -> rectifyAffineTransformationUpIsUp
//            (architectures.py:227-229,246-252, LAF.py:285-291); one thread per patch; optionally the shape filter of the row
//            (laf_ops.hip: aff_shape_filter_row) in the same kernel - the fused pipeline's finish + filter
//   OriNet : + bias -> tanh -> mean over the 3x3 map -> atan2 -> rotation (architectures.py:56-58,76-82, LAF.py:276-283); one
//            WAVEFRONT per patch: lane q < 18 adds the eight partials of tap q (18 consecutive floats per wave partial: coalesced;
//            one thread per patch read 144 floats at a 576-byte stride, 5.8x overfetch, 18 us for 2000 patches), the nine tanh
//            values of each output are added in tap order as before; optionally LAF <- LAF * R in the same kernel
//            (SparseImgRepresenter.py:173-177).
struct ShapeFuse {           // finish + shape filter in one kernel (pointers of image 0; strides like shape_filter_kernel)
    const float* resp; const float* lafs; float* key; int32_t* good; int32_t* cnt;
};
__global__ __launch_bounds__(256) void affnet_finish_kernel(const float* __restrict__ part, const float* __restrict__ hb,
                                                            const int32_t* __restrict__ count, int n_max, float* __restrict__ out, int row_begin,
                                                            int row_end, const int32_t* __restrict__ skip_cnt, int skip_n, ShapeFuse sf) {
    const int row = row_begin + blockIdx.x * 256 + threadIdx.x;
    const int n_img = count ? min(count[blockIdx.y], n_max) : n_max;
    const int n = min(n_img, row_end);
    const bool skip = lazy_skip(skip_cnt, skip_n, blockIdx.y);
    const size_t pidx = (size_t)blockIdx.y * n_max + row;
    if (sf.key) {
        if (blockIdx.x == 0 && threadIdx.x == 0)
            sf.cnt[(size_t)blockIdx.y * CNT_TOTAL + CNT_AFF_EVAL] = skip ? min(n_img, row_begin) : min(n_img, row_end);
        if (skip && row < n) { sf.key[pidx] = 0.0f; sf.good[pidx] = 0; }      // never evaluated: "not good" (no separate clearing pass)
    }
    if (row >= n || skip) return;
    float* o = out + 4 * pidx;
    const f32x4* pp = reinterpret_cast<const f32x4*>(part + pidx * HEAD_PART_AFF);
    f32x4 r[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) r[w] = pp[w];
    const f32x4 s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    const float x0 = tanhf(s.x + hb[0]), x1 = tanhf(s.y + hb[1]), x2 = tanhf(s.z + hb[2]);
    const float a00 = 1.0f + x0, a01 = 0.0f * x0, a10 = x1, a11 = 1.0f + x2;
    const float det = sqrtf(fabsf(a00 * a11 - a10 * a01 + 1e-10f));
    const float b2a2 = sqrtf(a01 * a01 + a00 * a00);
    const float o0 = b2a2 / det, o1 = 0.0f * det, o2 = (a11 * a01 + a10 * a00) / (b2a2 * det), o3 = det / b2a2;
    o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
    if (sf.key) {
        const size_t bi = blockIdx.y;
        aff_shape_filter_row(sf.resp + bi * n_max, sf.lafs + bi * n_max * 6, o0, o1, o2, o3, row, sf.key + bi * n_max, sf.good + bi * n_max,
                             sf.cnt + bi * CNT_TOTAL);
    }
}

__global__ __launch_bounds__(256) void orinet_finish_kernel(const float* __restrict__ part, const float* __restrict__ hb,
                                                            const int32_t* __restrict__ count, int n_max, float* __restrict__ out, int row_begin,
                                                            int row_end, float* __restrict__ rot_lafs, DenormSel ds) {
    const int row = row_begin + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int n = min(count ? min(count[blockIdx.y], n_max) : n_max, row_end);
    if (row >= n) {
        // fused denormalisation (denorm_level_select_kernel's convention): pixel frames past the row count are cleared
        if (ds.out_px && row < n_max && lane < 6) ds.out_px[6 * ((size_t)blockIdx.y * n_max + row) + lane] = 0.f;
        return;
    }
    const size_t pidx = (size_t)blockIdx.y * n_max + row;
    const float* pp = part + pidx * HEAD_PART_ORI;
    float th = 0.f;
    if (lane < 18) {
        float p[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) p[w] = pp[w * 18 + lane];
        float r = 0.f;
#pragma unroll
        for (int w = 0; w < 8; w += 2) r += p[w] + p[w + 1];
        th = tanhf(r + hb[lane >= 9 ? 1 : 0]);
    }
    float t0 = 0.f, t1 = 0.f;
#pragma unroll
    for (int q = 0; q < 9; ++q) { t0 += __shfl(th, q, 64); t1 += __shfl(th, 9 + q, 64); }
    if (lane != 0 && !(rot_lafs && ds.out_px)) return;                // (the fused level search below uses the whole wave: every lane carries the same row values)
    const float yv = t0 / 9.0f, xv = t1 / 9.0f;                       // AdaptiveAvgPool2d(1)
    const float ang = atan2f(yv + 1e-8f, xv + 1e-8f);                 // architectures.py:78
    const float sn = sinf(ang), cs = cosf(ang);
    float* o = out + 4 * pidx;
    if (lane == 0) { o[0] = cs; o[1] = sn; o[2] = -sn; o[3] = cs; }
    if (rot_lafs) {                                                   // apply_rotation_kernel (laf_ops.hip), same fmaf order
        float* L = rot_lafs + 6 * pidx;
        const float l00 = L[0], l01 = L[1], l10 = L[3], l11 = L[4], lx = L[2], ly = L[5];
        const float r0 = fmaf(l01, -sn, l00 * cs), r1 = fmaf(l01, cs, l00 * sn), r3 = fmaf(l11, -sn, l10 * cs), r4 = fmaf(l11, cs, l10 * sn);
        // the one-image latency path: denormalisation + pyramid-level choice of the row right here (was a launch of its own; same values, the level search
        // spread over the wave).  Every lane has read the frame BEFORE lane 0 overwrites it.
        if (ds.out_px)
            aff_denorm_level_row_wave(lane, r0, r1, lx, r3, r4, ly, ds.c_a, ds.c_x, ds.c_y, ds.ps, ds.lt, ds.ca, ds.cx, ds.cy, ds.out_px + 6 * pidx, ds.ids + 3 * pidx,
                                      ds.lafs_norm + 6 * pidx);
        if (lane == 0) { L[0] = r0; L[1] = r1; L[3] = r3; L[4] = r4; }
    }
}

// ---- HardNet head: (n x 8192) x (8192 x 128) GEMM + BN bias + L2 normalisation ----------------------
// Split-K GEMM on the fp32 matrix cores.  One workgroup = 256 threads = 64 patches x 128 outputs x one quarter of K
// (2048): wave w owns N-tiles 2w, 2w+1 for all four 16-patch M-tiles (8 accumulators).  K is walked in the conv loops'
// interleaved order (k = 16 G + 4 kq + j belongs to k-step j of lane group kq), so per 16 k a wave issues 4
// ds_read_b128 (A, from the LDS slab) + 2 buffer_load_dwordx4 (B, BN-folded weights [k/16][kq][n][4] from L2) for 32
// MFMAs.  The A slab (64 x 128) is fetched one iteration ahead into registers (buffer loads: rows >= n read as zero)
// and written to LDS with 16-byte stores.  Partial sums go to a scratch [4][n][128] with plain stores (no float atomics:
// bit-reproducible); hardnet_finish_kernel adds them in fixed order, adds the bias and L2-normalises.
#define HEAD_KSPLIT 4
#define HEAD_KC 128
#define HEAD_AS (HEAD_KC + 4)    // row stride: 16-byte aligned rows
// MP = patches per workgroup: 64 (4 M-tiles per wave) is the throughput shape; 32 / 16 give small calls 2x / 4x as many workgroups
// (one image with 2000 keypoints is 32 x 4 workgroups of the 64-patch shape on 256 CUs: 85 us at 49 TFLOP/s).  The K order of every
// output's sum is the same for all three, so results do not depend on the shape.
template <int MP>
__global__ __launch_bounds__(256, 2) void hardnet_head_kernel(const float* __restrict__ trunk, const float* __restrict__ Bw,
                                                              const int32_t* __restrict__ count, int n_max, float* __restrict__ partial) {
    constexpr int MI = MP / 16;                  // M-tiles per wave
    constexpr int NA = MP * HEAD_KC / 4 / 256;   // float4 of the A slab per thread
    __shared__ __attribute__((aligned(16))) float As[MP * HEAD_AS];
    const int n = count ? min(count[blockIdx.z], n_max) : n_max;      // blockIdx.z = image of the batch
    const int p0 = blockIdx.x * MP;
    if (p0 >= n) return;
    const size_t rows_total = (size_t)gridDim.z * n_max;
    const int kbeg = blockIdx.y * (HEAD_K / HEAD_KSPLIT);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t rA = weight_rsrc(trunk + (size_t)blockIdx.z * n_max * HEAD_K, n * HEAD_K);   // rows >= n -> 0
    const __amdgpu_buffer_rsrc_t rB = weight_rsrc(Bw, HEAD_K * 128);
    int offA[NA];
#pragma unroll
    for (int r = 0; r < NA; ++r) {
        const int f = tid + 256 * r, row = f >> 5, c4 = f & 31;       // 32 consecutive float4 = one 512-byte row segment
        offA[r] = ((p0 + row) * HEAD_K + 4 * c4) * 4;
    }
    const int offB = ((kq * 128) + wave * 32 + m) * 16;
    const unsigned a_addr = lds_byte_addr(As) + (m * HEAD_AS + 4 * kq) * 4;
    f32x4 acc[MI][2], stage[NA];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NA; ++r) stage[r] = buf_read4(rA, offA[r], kbeg * 4);
#pragma unroll 1
    for (int k0 = kbeg; k0 < kbeg + HEAD_K / HEAD_KSPLIT; k0 += HEAD_KC) {
        __syncthreads();                                              // the previous slab has been consumed
#pragma unroll
        for (int r = 0; r < NA; ++r) {
            const int f = tid + 256 * r, row = f >> 5, c4 = f & 31;
            *reinterpret_cast<f32x4*>(&As[row * HEAD_AS + 4 * c4]) = stage[r];
        }
        __syncthreads();
        if (k0 + HEAD_KC < kbeg + HEAD_K / HEAD_KSPLIT) {
#pragma unroll
            for (int r = 0; r < NA; ++r) stage[r] = buf_read4(rA, offA[r], (k0 + HEAD_KC) * 4);
        }
        f32x4 fa[2][MI], fb[2][2];
#pragma unroll
        for (int i = 0; i < MI; ++i) fa[0][i] = lds_read4(a_addr + i * 16 * HEAD_AS * 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[0][j] = buf_read4(rB, offB + j * 256, k0 * 512);
#pragma unroll
        for (int g = 0; g < HEAD_KC / 16; ++g) {
            const int cur = g & 1, nxt = cur ^ 1;
            if (g + 1 < HEAD_KC / 16) {
#pragma unroll
                for (int i = 0; i < MI; ++i) fa[nxt][i] = lds_read4(a_addr + i * 16 * HEAD_AS * 4 + (g + 1) * 64);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[nxt][j] = buf_read4(rB, offB + j * 256, (k0 + 16 * (g + 1)) * 512);
            }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[cur][i][s4], fb[cur][j][s4], acc[i][j], 0, 0, 0);
        }
    }
    // acc[i][j][r]: patch p0 + 16 i + 4 (lane>>4) + r, channel 32 wave + 16 j + (lane & 15)
    const int g = lane >> 4;
    float* dst = partial + ((size_t)blockIdx.y * rows_total + (size_t)blockIdx.z * n_max) * 128;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = p0 + 16 * i + 4 * g + r;
            if (row >= n) continue;
            dst[(size_t)row * 128 + wave * 32 + m] = acc[i][0][r];
            dst[(size_t)row * 128 + wave * 32 + 16 + m] = acc[i][1][r];
        }
}

// The same GEMM on split operands (AFFNET_ARITH_FP32_SPLIT3): the A slab is split ONCE per element while it is staged into LDS (each conv5
// element belongs to exactly one workgroup: M-tile x K-quarter), stored as term-interleaved 48-byte cells of 8 consecutive k
// (row pitch 128 k * 6 B + 16 B: the 16 rows of an M-tile fall into 16 different 16-byte bank slots), B = the pre-split head weights
// [k / 32][term][kq][n][8] straight from L2.  Six v_mfma_f32_16x16x32_bf16 per fp32 product in term-major order, fp32 accumulate; same
// partial-sum scratch and finish kernel as the exact path.
// TERMS = 2 (AFFNET_ARITH_FP32_SPLIT2H): two fp16 terms, three v_mfma_f32_16x16x32_f16 per product, the same cells with the third slot unused; the head
// weights are packed times 2^e, the partial sums are multiplied by 2^-e (behind the weights) before they are stored.
#define HEAD_S3_ROWB (HEAD_KC * 6 + 16)
template <int MP, int TERMS = 3>
__global__ __launch_bounds__(256, 2) void hardnet_head_s3_kernel(const float* __restrict__ trunk, const float* __restrict__ Bw3,
                                                                 const int32_t* __restrict__ count, int n_max, float* __restrict__ partial) {
    constexpr int MI = MP / 16;
    constexpr int NA = MP * HEAD_KC / 4 / 256;
    __shared__ __attribute__((aligned(16))) char As[MP * HEAD_S3_ROWB];
    const int n = count ? min(count[blockIdx.z], n_max) : n_max;
    const int p0 = blockIdx.x * MP;
    if (p0 >= n) return;
    const size_t rows_total = (size_t)gridDim.z * n_max;
    const int kbeg = blockIdx.y * (HEAD_K / HEAD_KSPLIT);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t rA = weight_rsrc(trunk + (size_t)blockIdx.z * n_max * HEAD_K, n * HEAD_K);   // rows >= n -> 0
    const __amdgpu_buffer_rsrc_t rB = weight_rsrc(Bw3, HEAD_K * 128 * TERMS / 2);
    int offA[NA];
#pragma unroll
    for (int r = 0; r < NA; ++r) {
        const int f = tid + 256 * r, row = f >> 5, c4 = f & 31;
        offA[r] = ((p0 + row) * HEAD_K + 4 * c4) * 4;
    }
    const int offB = ((kq * 128) + wave * 32 + m) * 16;
    const unsigned a_addr = lds_byte_addr(reinterpret_cast<const float*>(As)) + m * HEAD_S3_ROWB + kq * 48;
    f32x4 acc[MI][2], stage[NA];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NA; ++r) stage[r] = buf_read4(rA, offA[r], kbeg * 4);
#pragma unroll 1
    for (int k0 = kbeg; k0 < kbeg + HEAD_K / HEAD_KSPLIT; k0 += HEAD_KC) {
        __syncthreads();                                              // the previous slab has been consumed
#pragma unroll
        for (int r = 0; r < NA; ++r) {
            const int f = tid + 256 * r, row = f >> 5, c4 = f & 31;
            char* dst = As + row * HEAD_S3_ROWB + (c4 >> 1) * 48 + (c4 & 1) * 8;      // cell = 8 consecutive k, this float4 = its lower / upper half
            split_store4<TERMS>(dst, stage[r]);
        }
        __syncthreads();
        if (k0 + HEAD_KC < kbeg + HEAD_K / HEAD_KSPLIT) {
#pragma unroll
            for (int r = 0; r < NA; ++r) stage[r] = buf_read4(rA, offA[r], (k0 + HEAD_KC) * 4);
        }
        bf16x8 fb[2][TERMS][2];                                       // [buffer][term][N-tile]
        auto load_b = [&](int buf, int ks) {
#pragma unroll
            for (int t = 0; t < TERMS; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    fb[buf][t][j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rB, offB + j * 256, ((ks * TERMS + t) * 4 * 128) * 16, 0));
        };
        load_b(0, k0 >> 5);
#pragma unroll
        for (int s = 0; s < HEAD_KC / 32; ++s) {
            const int cur = s & 1;
            if (s + 1 < HEAD_KC / 32) load_b(cur ^ 1, (k0 >> 5) + s + 1);
            bf16x8 fa[MI][TERMS];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int t = 0; t < TERMS; ++t) fa[i][t] = __builtin_bit_cast(bf16x8, lds_read4(a_addr + i * 16 * HEAD_S3_ROWB + s * 192 + t * 16));
            // term pairs (a_i, b_j), i + j <= TERMS - 1, term-major
            constexpr int NPAIR = TERMS == 3 ? 6 : 3;
            constexpr int TA3[6] = {0, 0, 0, 1, 1, 2}, TB3[6] = {0, 1, 2, 0, 1, 0}, TA2[3] = {0, 0, 1}, TB2[3] = {0, 1, 0};
#pragma unroll
            for (int q = 0; q < NPAIR; ++q)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = split_mfma<TERMS>(fa[i][TERMS == 3 ? TA3[q] : TA2[q]], fb[cur][TERMS == 3 ? TB3[q] : TB2[q]][j], acc[i][j]);
        }
    }
    if constexpr (TERMS == 2) {
        const float osc = Bw3[(size_t)HEAD_K * 128];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] *= osc;
    }
    // acc[i][j][r]: patch p0 + 16 i + 4 (lane>>4) + r, channel 32 wave + 16 j + (lane & 15)
    const int g = lane >> 4;
    float* dst = partial + ((size_t)blockIdx.y * rows_total + (size_t)blockIdx.z * n_max) * 128;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = p0 + 16 * i + 4 * g + r;
            if (row >= n) continue;
            dst[(size_t)row * 128 + wave * 32 + m] = acc[i][0][r];
            dst[(size_t)row * 128 + wave * 32 + 16 + m] = acc[i][1][r];
        }
}

// One wavefront per patch: sum the K-split partials in fixed order, + BN bias, L2 normalise (eps 1e-8).  Rows past the image's row
// count are cleared here (the caller's descriptor buffer needs no separate fill).
__global__ __launch_bounds__(256) void hardnet_finish_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                                             const int32_t* __restrict__ count, int n_max, float* __restrict__ out) {
    const int n = count ? min(count[blockIdx.y], n_max) : n_max;      // blockIdx.y = image of the batch
    const int lrow = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (lrow >= n_max) return;
    const size_t rows_total = (size_t)gridDim.y * n_max, row = (size_t)blockIdx.y * n_max + lrow;
    if (lrow >= n) { out[row * 128 + lane] = 0.0f; out[row * 128 + 64 + lane] = 0.0f; return; }
    float v0 = 0.f, v1 = 0.f;
#pragma unroll
    for (int s = 0; s < HEAD_KSPLIT; ++s) {
        const float* p = partial + ((size_t)s * rows_total + row) * 128;
        v0 += p[lane]; v1 += p[64 + lane];
    }
    v0 += bias[lane]; v1 += bias[64 + lane];
    const float tot = wave_sum(v0 * v0 + v1 * v1);
    const float nrm = sqrtf(tot + 1e-8f);                                  // L2Norm (HardNet.py:15-18)
    out[row * 128 + lane] = v0 / nrm;
    out[row * 128 + 64 + lane] = v1 / nrm;
}

// ---- host entry points -------------------------------------------------------------------------------
static void aff_fill_pyr_src(const affnet_ctx* ctx, PyrSrc* s) {
    memset(s, 0, sizeof(*s));                            // no workspace bound (patch-tensor calls): an all-zero table
    if (ctx->ws) aff_fill_pyr_table(ctx, &s->t);
    aff_base_grid(32, s->base);
}

// One CNN call: trunk launch + the net's finish stage.  Callers set the fields they mean by name; the rest keep these defaults.
struct CnnCall {
    int kind = -1;                                                   // AFFNET_NET_AFFNET / _ORINET / _HARDNET
    const float* packed = nullptr;
    const float* patches = nullptr;                                  // (n,32,32), or NULL: sample from the pyramid with lafs / ids
    const float* lafs = nullptr; const int32_t* ids = nullptr;
    const int32_t* count = nullptr; int n_max = 0;
    float* out = nullptr; float* scratch = nullptr;
    hipStream_t st = nullptr;
    int dbg_layer = -1; float* dbg_out = nullptr;                    // layer >= 0: dump this trunk layer of patch 0, no finish stage
    bool mark_head = false;                                          // stage mark 7 between trunk and head (affnet_describe_detected)
    int row_begin = 0, row_count = -1;                               // row window of every image; -1 = up to n_max
    const int32_t* skip_cnt = nullptr; int skip_n = 0;               // lazy-evaluation predicate (see CnnArgs)
    const ShapeFuse* fuse = nullptr; int shape_op = 0;               // AffNet: shape filter in the finish kernel, counter bookkeeping in the trunk
    float* rot_lafs = nullptr; const DenormSel* denorm = nullptr;    // OriNet: LAF <- LAF * R in the finish kernel (+ denormalisation and level choice)
};

// Argument checks, in this order.  *rows = rows per image to launch; 0 with AFFNET_OK = nothing to do.
static int cnn_check(affnet_ctx* ctx, const CnnCall& c, int* rows) {
    *rows = 0;
    if (c.kind < 0 || c.kind > 2) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: unknown net kind %d", c.kind);
    if (!c.packed || !c.out || c.n_max < 0 || (!c.patches && (!c.lafs || !c.ids))) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: null argument");
    if (!c.patches && !ctx->ws) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: sampling from the pyramid needs a bound workspace");
    if (c.dbg_layer < 0 && !c.scratch)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: d_scratch is required (HardNet n*(8192+512) floats, AffNet / OriNet n*144 floats)");
    if (c.dbg_layer >= 0 && ctx->arith != AFFNET_ARITH_FP32_MFMA)     // the split trunks have no per-layer dump: the exact kernel would answer
        return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: layer dumps exist for AFFNET_ARITH_FP32_MFMA only (context is in arithmetic mode %d)", ctx->arith);
    if (c.n_max == 0) return AFFNET_OK;
    if (c.kind == AFFNET_NET_HARDNET && c.n_max > 65535)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: n_max=%d (HardNet head: max 65535 rows per image)", c.n_max);
    const int row_count = c.row_count < 0 ? c.n_max - c.row_begin : c.row_count;
    if (c.row_begin < 0 || row_count < 0 || c.row_begin + row_count > c.n_max) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: bad row window");
    *rows = row_count;
    return AFFNET_OK;
}

// 0 = exact fp32, 1 = three bf16 terms, 2 = two fp16 terms: second index of the trunk and head kernel tables
static int arith_index(const affnet_ctx* ctx) {
    return ctx->arith == AFFNET_ARITH_FP32_SPLIT2H ? 2 : (ctx->arith == AFFNET_ARITH_FP32_SPLIT3 ? 1 : 0);
}

// The context's buffer of derived Winograd weights (Wino16::FLOATS per 16-channel net).  Allocated on first use; affnet_graph_capture_extract calls this
// before the capture begins (no allocation inside a capture).
int aff_wino_u_ensure(affnet_ctx* ctx) {
    if (ctx->wino_u) return AFFNET_OK;
    AFF_HIP(ctx, hipMalloc((void**)&ctx->wino_u, (size_t)2 * Wino16::FLOATS * sizeof(float)));
    return AFFNET_OK;
}

// U of conv1 / conv3 / conv5 of `packed` (AffNet or OriNet blob) into the context's region of that net, on the launch stream: 5376 threads, 194 KB read, 344 KB written.
// In front of EVERY exact OriNet trunk launch, so that a blob rewritten in place (load_state_dict into the same device buffer) can never meet
// stale weights, eagerly or in a replayed graph.
static int wino_derive_u(affnet_ctx* ctx, int kind, const float* packed, const NetLayout& L, hipStream_t st, const float** u) {
    const int rc = aff_wino_u_ensure(ctx);
    if (rc) return rc;
    float* dst = ctx->wino_u + (size_t)kind * Wino16::FLOATS;
    hipLaunchKernelGGL(wino_derive_u_kernel, dim3((Wino16::PAIRS + 255) / 256), dim3(256), 0, st, packed, (int)L.w_off[1], (int)L.w_off[3], (int)L.w_off[5], dst);
    AFF_LAUNCH_CHECK(ctx);
    *u = dst;
    return AFFNET_OK;
}

static int trunk_launch(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, dim3 grid) {
    CnnArgs a;
    a.packed = c.packed; a.off = to_offsets(L, ctx->arith);            // the split copy of the active mode
    a.wino_u = nullptr;
    if (c.kind == AFFNET_NET_ORINET && ctx->arith == AFFNET_ARITH_FP32_MFMA) {
        const int rc = wino_derive_u(ctx, c.kind, c.packed, L, c.st, &a.wino_u);
        if (rc) return rc;
    }
    a.patches = c.patches; a.lafs = c.lafs; a.ids = c.ids; a.count = c.count; a.n_max = c.n_max;
    a.out = (c.dbg_layer < 0) ? c.scratch : c.out;      // trunk kernels: HardNet conv5 tensor / AffNet, OriNet head partials
    a.dbg_layer = c.dbg_layer; a.dbg_out = c.dbg_out; a.dbg_time = ctx->dbg_time;
    a.row_begin = c.row_begin; a.skip_cnt = c.skip_cnt; a.skip_n = c.skip_n;
    a.shape_cnt = (c.fuse && c.shape_op) ? c.fuse->cnt : nullptr; a.shape_op = c.shape_op;
    a.s3_alt = ctx->split3_variant;
    PyrSrc ps;
    aff_fill_pyr_src(ctx, &ps);
    // (Tried and removed: two AffNet patches per persistent 16-wave workgroup in anti-phase - correct but 8 % slower, the
    // small-tile loops reach 85-90 % of the pipe rate with two waves per SIMD; 16-wave HardNet workgroups - slower too.)
    // trunk instantiation [net kind][exact, three bf16 terms, two fp16 terms][phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check)
    static_assert(AFFNET_NET_AFFNET == 0 && AFFNET_NET_ORINET == 1 && AFFNET_NET_HARDNET == 2, "trunk table order");
    static void (*const trunks[3][3][2])(CnnArgs, PyrSrc) = {
        {{cnn32_trunk_kernel<0, 8, false>, cnn32_trunk_kernel<0, 8, true>}, {cnn32_trunk_kernel<0, 8, false, 3>, cnn32_trunk_kernel<0, 8, true, 3>},
         {cnn32_trunk_kernel<0, 8, false, 2>, cnn32_trunk_kernel<0, 8, true, 2>}},
        {{cnn32_trunk_kernel<1, 8, false>, cnn32_trunk_kernel<1, 8, true>}, {cnn32_trunk_kernel<1, 8, false, 3>, cnn32_trunk_kernel<1, 8, true, 3>},
         {cnn32_trunk_kernel<1, 8, false, 2>, cnn32_trunk_kernel<1, 8, true, 2>}},
        {{cnn32_trunk_kernel<2, 8, false>, cnn32_trunk_kernel<2, 8, true>}, {cnn32_trunk_kernel<2, 8, false, 3>, cnn32_trunk_kernel<2, 8, true, 3>},
         {cnn32_trunk_kernel<2, 8, false, 2>, cnn32_trunk_kernel<2, 8, true, 2>}}};
    hipLaunchKernelGGL(trunks[c.kind][arith_index(ctx)][a.dbg_time || c.dbg_layer >= 0], grid, dim3(512), 0, c.st, a, ps);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// AffNet / OriNet: combine the per-wave head partials in `scratch` (rows of the window)
static int finish_affnet(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int rows, int B) {
    ShapeFuse sf;
    memset(&sf, 0, sizeof(sf));
    if (c.fuse) sf = *c.fuse;
    hipLaunchKernelGGL(affnet_finish_kernel, dim3(aff_cdiv(rows, 256), B), dim3(256), 0, c.st, c.scratch, c.packed + L.head_b, c.count, c.n_max, c.out,
                       c.row_begin, c.row_begin + rows, c.skip_cnt, c.skip_n, sf);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

static int finish_orinet(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int rows, int B) {
    DenormSel ds;
    memset(&ds, 0, sizeof(ds));
    if (c.denorm && c.rot_lafs) ds = *c.denorm;
    hipLaunchKernelGGL(orinet_finish_kernel, dim3(aff_cdiv(rows, 4), B), dim3(256), 0, c.st, c.scratch, c.packed + L.head_b, c.count, c.n_max, c.out,
                       c.row_begin, c.row_begin + rows, c.rot_lafs, ds);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// HardNet: head GEMM over all rows of the trunk output in `scratch` + finish kernel
static int hardnet_head(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int B) {
    const int n_max = c.n_max;
    float* partial = c.scratch + (size_t)B * n_max * HEAD_K;   // [HEAD_KSPLIT][B * n_max][128] behind the trunk output
    // patches per workgroup: the 64-patch shape once it gives every CU a workgroup, else 32 / 16 (same sums, more workgroups)
    int mp = (aff_cdiv(n_max, 64) * HEAD_KSPLIT * B >= 256) ? 64 : ((aff_cdiv(n_max, 32) * HEAD_KSPLIT * B >= 256) ? 32 : 16);
    if (const char* e = getenv("AFFNET_HEAD_MP")) { const int v = atoi(e); if (v == 16 || v == 32 || v == 64) mp = v; }   // tuning aid
    // head instantiation [exact, three bf16 terms, two fp16 terms][MP 64, 32, 16]; the split modes run the head GEMM on split operands as well
    static void (*const heads[3][3])(const float*, const float*, const int32_t*, int, float*) = {
        {hardnet_head_kernel<64>, hardnet_head_kernel<32>, hardnet_head_kernel<16>},
        {hardnet_head_s3_kernel<64, 3>, hardnet_head_s3_kernel<32, 3>, hardnet_head_s3_kernel<16, 3>},
        {hardnet_head_s3_kernel<64, 2>, hardnet_head_s3_kernel<32, 2>, hardnet_head_s3_kernel<16, 2>}};
    const int ai = arith_index(ctx);
    const float* hw = c.packed + (ai == 2 ? L.head_h2 : (ai == 1 ? L.head_s3 : L.head_w));
    hipLaunchKernelGGL(heads[ai][mp == 64 ? 0 : (mp == 32 ? 1 : 2)], dim3(aff_cdiv(n_max, mp), HEAD_KSPLIT, B), dim3(256), 0, c.st, c.scratch, hw, c.count,
                       n_max, partial);
    AFF_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(hardnet_finish_kernel, dim3(aff_cdiv(n_max, 4), B), dim3(256), 0, c.st, partial, c.packed + L.head_b, c.count, n_max, c.out);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

static int cnn_launch(affnet_ctx* ctx, const CnnCall& c) {
    int rows;
    int rc = cnn_check(ctx, c, &rows);
    if (rc || rows == 0) return rc;
    const NetLayout L = net_layout(c.kind);
    const int B = c.patches ? 1 : ctx->B;                // patch tensors are single-"image"; pyramid sampling covers the batch
    rc = trunk_launch(ctx, c, L, dim3(rows, B));
    if (rc) return rc;
    if (c.dbg_layer < 0 && c.kind != AFFNET_NET_HARDNET) {
        rc = c.kind == AFFNET_NET_AFFNET ? finish_affnet(ctx, c, L, rows, B) : finish_orinet(ctx, c, L, rows, B);
        if (rc) return rc;
    }
    if (c.mark_head) aff_prof_mark(ctx, 7, c.st);
    if (c.dbg_layer < 0 && c.kind == AFFNET_NET_HARDNET) return hardnet_head(ctx, c, L, B);
    return AFFNET_OK;
}

extern "C" int affnet_cnn32_forward(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patches, const int32_t* d_count,
                                    int n_max, float* d_out, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_patches) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32_forward: null argument");
    CnnCall c;
    c.kind = net_kind; c.packed = d_packed; c.patches = d_patches; c.count = d_count; c.n_max = n_max; c.out = d_out; c.scratch = d_scratch; c.st = (hipStream_t)stream;
    return cnn_launch(ctx, c);
}

extern "C" int affnet_cnn32_forward_pyr(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_lafs, const int32_t* d_ids,
                                        const int32_t* d_count, int n_max, float* d_out, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx) return AFFNET_ERR_INVALID;
    CnnCall c;
    c.kind = net_kind; c.packed = d_packed; c.lafs = d_lafs; c.ids = d_ids; c.count = d_count; c.n_max = n_max; c.out = d_out; c.scratch = d_scratch; c.st = (hipStream_t)stream;
    return cnn_launch(ctx, c);
}

// AffNet on a row window with the shape filter of every evaluated row fused into the finish kernel (key / good / survivor count in
// the context's stage buffers) and the shape-stage counter bookkeeping done by the trunk launch (shape_op: see CnnArgs); lazy = under
// the lazy-evaluation predicate.
int aff_affnet_filter_rows(affnet_ctx* ctx, const float* packed, const float* resp, const float* lafs, const int32_t* ids, const int32_t* count,
                           float* out, float* scratch, int row_begin, int row_count, bool lazy, int shape_op, hipStream_t st) {
    ShapeFuse sf;
    sf.resp = resp; sf.lafs = lafs; sf.key = ctx->st_key; sf.good = ctx->st_good; sf.cnt = ctx->cnt;
    CnnCall c;
    c.kind = AFFNET_NET_AFFNET; c.packed = packed; c.lafs = lafs; c.ids = ids; c.count = count; c.n_max = ctx->cap_pre; c.out = out; c.scratch = scratch; c.st = st;
    c.row_begin = row_begin; c.row_count = row_count;
    c.skip_cnt = lazy ? ctx->cnt : nullptr; c.skip_n = ctx->cfg.num_features;
    c.fuse = &sf; c.shape_op = shape_op;
    return cnn_launch(ctx, c);
}

// OriNet with LAF <- LAF * R applied by the finish kernel (d_lafs rotated in place).
// denorm != NULL: the finish kernel also denormalises the rotated frame, chooses its pyramid level and writes the re-normalised frame (aff_denorm_level_select's
// work, one launch less per call).
int aff_orinet_rotate(affnet_ctx* ctx, const float* packed, float* lafs, const int32_t* ids, const int32_t* count, int n_max, float* out, float* scratch,
                      hipStream_t st, const DenormSel* denorm) {
    CnnCall c;
    c.kind = AFFNET_NET_ORINET; c.packed = packed; c.lafs = lafs; c.ids = ids; c.count = count; c.n_max = n_max; c.out = out; c.scratch = scratch; c.st = st;
    c.rot_lafs = lafs; c.denorm = denorm;
    return cnn_launch(ctx, c);
}

int aff_hardnet_forward_pyr_marked(affnet_ctx* ctx, const float* packed, const float* lafs, const int32_t* ids, const int32_t* count,
                                   int n_max, float* out, float* scratch, hipStream_t st) {
    CnnCall c;
    c.kind = AFFNET_NET_HARDNET; c.packed = packed; c.lafs = lafs; c.ids = ids; c.count = count; c.n_max = n_max; c.out = out; c.scratch = scratch; c.st = st;
    c.mark_head = true;
    return cnn_launch(ctx, c);
}

extern "C" int affnet_debug_split3_variant(affnet_ctx* ctx, int bits) {
    if (!ctx) return AFFNET_ERR_INVALID;
    ctx->split3_variant = bits;             // bit 0: HardNet loops with alternating wave priorities (A/B aid; default off since round 4)
    return AFFNET_OK;
}

extern "C" int affnet_cnn32_debug_timing(affnet_ctx* ctx, unsigned long long* d_stamps) {
    if (!ctx) return AFFNET_ERR_INVALID;
    ctx->dbg_time = d_stamps;   // device buffer of n_patches * waves * 32 uint64, or NULL to switch the stamps off (this context only)
    return AFFNET_OK;
}

extern "C" int affnet_cnn32_debug_layer(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patch, int layer, float* d_out,
                                        void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_patch || !d_out || layer < 0 || layer > 5) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32_debug_layer: bad argument");
    CnnCall c;
    c.kind = net_kind; c.packed = d_packed; c.patches = d_patch; c.n_max = 1; c.out = d_out; c.st = (hipStream_t)stream;
    c.dbg_layer = layer; c.dbg_out = d_out;
    return cnn_launch(ctx, c);
}

extern "C" int affnet_cnn32_debug_winograd_u(affnet_ctx* ctx, int net_kind, const float* d_packed, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_out || (net_kind != AFFNET_NET_AFFNET && net_kind != AFFNET_NET_ORINET) || (layer != 1 && layer != 3 && layer != 5))
        return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32_debug_winograd_u: AffNet / OriNet, layer 1, 3 or 5");
    const float* u;
    const int rc = wino_derive_u(ctx, net_kind, d_packed, net_layout(net_kind), (hipStream_t)stream, &u);
    if (rc) return rc;
    return aff_copy_async(ctx, d_out, u + Wino16::offset(layer), (size_t)Wino16::floats(layer) * sizeof(float), (hipStream_t)stream);
}

#ifdef AFFNET_PROBES   // libaffnet_hip_probes.so only (include/affnet_hip_probes.h)
// ---- tuning aid: one HardNet layer's MFMA loop in isolation (no barriers, no epilogue), repeated ----------------------
template <int LAYER, int PROBE>
__global__ __launch_bounds__(512, 2) void cnn32_probe_kernel(const float* __restrict__ packed, NetOffsets off, int reps, float* __restrict__ out) {
    constexpr int CB = 32, NW = 8;
    __shared__ __attribute__((aligned(16))) float lds[TrunkLds<CB>::TOTAL];     // same footprint as the trunk: 1 workgroup / CU
    for (int i = threadIdx.x; i < TrunkLds<CB>::TOTAL; i += 512) lds[i] = 0.001f * (float)(i & 255);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float sink = 0.f;
    if (PROBE & 4) asm volatile("; accumulators in AGPRs" ::"a"(sink));     // any 'a' operand switches the MFMAs to their AGPR form
    for (int r = 0; r < reps; ++r) {
        if (LAYER == 1) {
            f32x4 acc[8][2], b0[1][2];
            prefetch_b0<NW, CB, 32, 8, 2, 1>(packed + off.w[1], b0, wave, lane);
            conv3x3_mfma<NW, CB, CB, LayC0, 1, 8, 2, 1, (PROBE & 11)>(lds, packed + off.w[1], b0, acc, wave, lane);
#pragma unroll
            for (int i = 0; i < 8; ++i) sink += acc[i][0][0] + acc[i][1][3];
        } else {
            f32x4 acc[4][1], b0[2][1];
            prefetch_b0<NW, 4 * CB, 8, 4, 1, 2>(packed + off.w[5], b0, wave, lane);
            conv3x3_mfma<NW, 4 * CB, 4 * CB, LayC4, 1, 4, 1, 2, (PROBE & 11)>(lds, packed + off.w[5], b0, acc, wave, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i) sink += acc[i][0][0] + acc[i][0][3];
        }
    }
    if (sink == 12345.678f) out[0] = sink;
    if (threadIdx.x == 0 && blockIdx.x == 0) out[1] = sink;
}

// Same for the 16-channel trunks (AffNet / OriNet shapes, 79 KB of LDS -> two workgroups per CU, 128 VGPRs).
template <int LAYER, int PROBE>
__global__ __launch_bounds__(512, 4) void cnn16_probe_kernel(const float* __restrict__ packed, NetOffsets off, int reps, float* __restrict__ out) {
    constexpr int CB = 16, NW = 8;
    __shared__ __attribute__((aligned(16))) float lds[TrunkLds<CB>::TOTAL];
    for (int i = threadIdx.x; i < TrunkLds<CB>::TOTAL; i += 512) lds[i] = 0.001f * (float)(i & 255);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float sink = 0.f;
    for (int r = 0; r < reps; ++r) {
        if (LAYER == 3) {
            f32x4 acc[2][2], b0[2][2];
            prefetch_b0<NW, 2 * CB, 16, 2, 2, 2>(packed + off.w[3], b0, wave, lane);
            conv3x3_mfma<NW, 2 * CB, 2 * CB, LayC2, 1, 2, 2, 2, PROBE>(lds, packed + off.w[3], b0, acc, wave, lane);
            sink += acc[0][0][0] + acc[1][1][3] + acc[0][1][1] + acc[1][0][2];
        } else if (LAYER == 4) {    // conv3 again, 4 pixel tiles x 1 channel tile per wave: half the weight loads per MFMA
            f32x4 acc[4][1], b0[1][1];
            prefetch_b0<NW, 2 * CB, 16, 4, 1, 1>(packed + off.w[3], b0, wave, lane);
            conv3x3_mfma<NW, 2 * CB, 2 * CB, LayC2, 1, 4, 1, 1, PROBE>(lds, packed + off.w[3], b0, acc, wave, lane);
            sink += acc[0][0][0] + acc[1][0][3] + acc[2][0][1] + acc[3][0][2];
        } else {
            f32x4 acc[2][1], b0[2][1];
            prefetch_b0<NW, 4 * CB, 8, 2, 1, 2>(packed + off.w[5], b0, wave, lane);
            conv3x3_mfma<NW, 4 * CB, 4 * CB, LayC4, 1, 2, 1, 2, PROBE>(lds, packed + off.w[5], b0, acc, wave, lane);
            sink += acc[0][0][0] + acc[1][0][3];
        }
    }
    if (sink == 12345.678f) out[0] = sink;
    if (threadIdx.x == 0 && blockIdx.x == 0) out[1] = sink;
}

// layer: 1 (HardNet conv1, TM 8 x TN 2), 5 (HardNet conv5, TM 4 x TN 1, 2 groups / chunk) with HardNet's packed weights;
// 13 / 15 (AffNet conv3, TM 2 x TN 2 / conv5, TM 2 x TN 1) with AffNet's.  probe: PROBE bits; d_out: 2 floats.
extern "C" int affnet_cnn32_probe(const float* d_packed_hardnet, int layer, int probe, int reps, int n_blocks, float* d_out, void* stream) {
    if (!d_packed_hardnet || !d_out || probe < 0 || probe > 15) return AFFNET_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (layer == 13 || layer == 14 || layer == 15) {
        if (probe > 3) return AFFNET_ERR_INVALID;
        const NetOffsets off16 = to_offsets(net_layout(AFFNET_NET_AFFNET));
#define PROBE16(L, P) if (layer == 10 + L && probe == P) hipLaunchKernelGGL((cnn16_probe_kernel<L, P>), dim3(n_blocks), dim3(512), 0, st, d_packed_hardnet, off16, reps, d_out)
        PROBE16(3, 0); PROBE16(3, 1); PROBE16(3, 2); PROBE16(3, 3); PROBE16(4, 0); PROBE16(4, 1); PROBE16(4, 2); PROBE16(4, 3); PROBE16(5, 0); PROBE16(5, 1); PROBE16(5, 2); PROBE16(5, 3);
#undef PROBE16
        return hipGetLastError() == hipSuccess ? AFFNET_OK : AFFNET_ERR_HIP;
    }
    if (layer != 1 && layer != 5) return AFFNET_ERR_INVALID;
    const NetOffsets off = to_offsets(net_layout(AFFNET_NET_HARDNET));
#define PROBE_CASE(L, P) if (layer == L && probe == P) hipLaunchKernelGGL((cnn32_probe_kernel<L, P>), dim3(n_blocks), dim3(512), 0, st, d_packed_hardnet, off, reps, d_out)
    PROBE_CASE(1, 0); PROBE_CASE(1, 1); PROBE_CASE(1, 2); PROBE_CASE(1, 3); PROBE_CASE(1, 4); PROBE_CASE(1, 8); PROBE_CASE(1, 9);
    PROBE_CASE(5, 0); PROBE_CASE(5, 1); PROBE_CASE(5, 2); PROBE_CASE(5, 3); PROBE_CASE(5, 4); PROBE_CASE(5, 8); PROBE_CASE(5, 9);
#undef PROBE_CASE
    return hipGetLastError() == hipSuccess ? AFFNET_OK : AFFNET_ERR_HIP;
}

#endif  // AFFNET_PROBES

// ---- MFMA layout self-test ------------------------------------------------------------------------------
__global__ void mfma_selftest_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out) {
    const int lane = threadIdx.x, m = lane & 15, kq = lane >> 4;
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(A[m * 4 + kq], B[kq * 16 + m], c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(4 * kq + r) * 16 + m] = c[r];
}

extern "C" int affnet_selftest_mfma(const float* d_A, const float* d_B, float* d_out, void* stream) {
    if (!d_A || !d_B || !d_out) return AFFNET_ERR_INVALID;
    hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_A, d_B, d_out);
    return hipGetLastError() == hipSuccess ? AFFNET_OK : AFFNET_ERR_HIP;
}
