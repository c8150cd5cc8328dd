// Trunk kernel of the 32x32-patch CNNs (AffNetFast / OriNetFast / HardNet) for gfx950 on the fp32 matrix cores: cnn32_trunk_kernel and its
// device helpers.  Included by cnn_trunk_affnet.hip / cnn_trunk_orinet.hip / cnn_trunk_hardnet.hip (and cnn_trunk_hardnet_poly.hip / cnn_trunk_hardnet_f43.hip / cnn_trunk_hardnet_c5.hip / cnn_trunk_hardnet_c1.hip: HardNet forms 1 / 2 / 3 / 4), which instantiate one net's six kernels each
// (three arithmetic modes x product / stamped), and by cnn_probe.hip for the LDS footprint.  The kernel holds four bodies: exact HardNet (descriptor forms 0 / 1 / 2 / 3 / 4),
// exact AffNet / OriNet, split HardNet, split AffNet / OriNet.
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
//     step's reads and transform between this step's MFMAs) and conv5 (conv3x3_wino_mfma_shared_v: V shared through LDS), U from the blob; in descriptor form 2
//     conv3 as Winograd F(4x4, 3x3) (conv3x3_f43_mfma_shared_v: V shared through LDS, a wave pair per channel block), U derived in front of the launch;
//     OriNet's conv1 / conv3 (conv3x3_wino_mfma_rows, one row of four transform positions at a time on 128 registers; U derived from the
//     blob's taps by derive_u_kernel, derive_u.hip, in front of every launch) and conv5 (conv3x3_wino_mfma_half_rows: a wave pair per channel block, two position rows
//     each, one row exchanged through LDS in a fixed order, 2x2-pixel fragments straight into the head's LDS copy).  AffNet has both forms: the direct one
//     (S3 = 0) and one with OriNet's Winograd conv1 / conv3 / conv5 and the head straight from conv5's fragments (S3 = 1).  The shape filter behind AffNet turns on the last bits of its output for a few rows, so
//     the fused shape pass runs the Winograd form on every row and the direct form on the rows a margin rule flags (shape_filter.h, cnn32.hip).  The
//     split-operand modes (affnet_set_arith) run conv1..5 on bf16 / fp16 terms (conv3x3_mfma_s3q);
//   * activations live in ONE LDS buffer, channel-interleaved by 4 ((c/4)*PSG + pixel*4 + c%4): one ds_read_b128 per lane =
//     the activation operands of four k-steps, one ds_write_b128 per tile in the epilogue (bias + ReLU), written IN PLACE
//     over the layer's input after a barrier.  No HBM traffic between layers;
//   * packed weights (weights_layout.h: w_tap_index; packed on the host by weights_pack.hip) stream from L2 through a buffer descriptor
//     (one buffer_load_dwordx4 per lane = the weight operands of four k-steps), software-pipelined one chunk ahead, loads interleaved
//     between the MFMAs;
//   * heads: HardNet stores its conv5 tile [pixel][channel] to HBM and an 8192 x 128 split-K MFMA GEMM over all patches
//     (cnn_heads.hip: hardnet_head_kernel + hardnet_finish_kernel: BN bias + L2 norm) follows; AffNet / OriNet reduce their heads' dot
//     products per wave straight from the conv5 accumulators (head_partials, head_partials_wino, head_partials_ori_lds) and affnet_finish_kernel /
//     orinet_finish_kernel (cnn_heads.hip) combine the eight partials per patch in fixed order (tanh, rectification / atan2).
// Host side: cnn32.hip; the plain types both sides share (CnnArgs, PyrSrc, TRUNK_*, HEAD_PART_*) are in common.h, the derived weights' layouts (Wino16, Poly32, F43) in weights_layout.h.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"

#include "cnn_mfma.h"

// AffNet head, first half, straight from the conv5 accumulators (no conv5 tensor in HBM): a lane owns channels c4..c4+3 of pixel p of
// each of its tiles = one float4 of the head weights [o][pixel][channel]; it forms its share of the 3 outputs (conv 64 -> 3, 8x8 valid,
// architectures.py:227-229), the wave reduces them and lane 0 writes the wave's partial sums to part[wave][4].  The eight partials per
// patch are combined in fixed order by affnet_finish_kernel (bit-reproducible, no atomics).  OriNet's head (2 x 9 outputs, part[8][18]):
// head_partials_ori_lds below.
template <int TM>
__device__ __forceinline__ void head_partials(const float* __restrict__ hw, const f32x4 (&bias)[1], const f32x4 (&acc)[TM][1],
                                              float* __restrict__ part, int wave, int lane) {
    constexpr int MT = 4, MG = MT / TM;
    const int mg = wave % MG, ng = wave / MG;
    const int n = lane & 15, g = lane >> 4;
    const int c4 = ng * 16 + 4 * g;
    f32x4 v[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) v[i] = bias_relu(acc[i][0], bias[0]);
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

// The same head from the fragments of the Winograd conv5 (conv3x3_wino_mfma_half_rows + wino5_combine; AffNet shape form 1): lane (m, g) of wave 2 p + h holds
// y[k] = pre-activation channels 16 p + 4 g .. + 3 of pixel (2 (m >> 2) + h, 2 (m & 3) + k), k = 0, 1 - again one float4 of the head weights per (output, pixel).
// The weights do not depend on the activations: aff_head_weights_wino requests them in front of the combine's barrier (as ori_head_weights).  No LDS copy and
// no barrier of its own; lane-local order (pixel k, channel j), wave_sum, then affnet_finish_kernel's order over the waves: fixed for every patch and launch.
__device__ __forceinline__ void aff_head_weights_wino(const float* __restrict__ hw, f32x4 (&w)[3][2], int wave, int lane) {
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(hw, 3 * 4096);
    const int m = lane & 15, c4 = (wave >> 1) * 16 + 4 * (lane >> 4);
    const int pix = (2 * (m >> 2) + (wave & 1)) * 8 + 2 * (m & 3);
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int k = 0; k < 2; ++k) w[o][k] = buf_read4(r, (pix * 64 + c4) * 4, (o * 4096 + k * 64) * 4);
}
__device__ __forceinline__ void head_partials_wino(const f32x4 (&w)[3][2], f32x4 bias, const f32x4 (&y)[2], float* __restrict__ part, int wave, int lane) {
    f32x4 v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) v[k] = bias_relu(y[k], bias);
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        float sacc = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) sacc = fmaf(v[k][j], w[o][k][j], sacc);
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
// The direct form's head in one piece (the split-operand OriNet trunks): both halves as above.  The halo and the reduction are the pieces above; the lane's weight
// position, its weight loads and the pbase / interior-store loop are kept as one body so that those kernels' code does not move (with OriHeadLane + ori_head_weights:
// 11 / 4 of 3568 / 3822 disassembly lines of the two-term / three-term kernel, with ori_head_pbase besides 13 / 6; profiles/trunk_merge_report.md).
template <int TM, int NTHR>
__device__ __forceinline__ void head_partials_ori_lds(const float* __restrict__ hw, const f32x4 (&bias)[1], const f32x4 (&acc)[TM][1],
                                                      float* __restrict__ part, float* act, int wave, int lane, int tid) {
    constexpr int MT = 4, MG = MT / TM;
    const int mg = wave % MG, ng = wave / MG;
    const int n = lane & 15, g = lane >> 4;
    const int c4 = ng * 16 + 4 * g;
    f32x4 v[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) v[i] = bias_relu(acc[i][0], bias[0]);
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(hw, 2 * 4096);
    f32x4 w[2][TM];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int i = 0; i < TM; ++i) w[o][i] = buf_read4(r, (n * 64 + c4) * 4, (o * 4096 + (mg * TM + i) * 16 * 64) * 4);
    __syncthreads();                                                     // every wave has finished reading the conv5 input from `act`
    ori_head_zero_halo<NTHR>(act, tid);
    int pbase[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int p = (mg * TM + i) * 16 + n;
        pbase[i] = ((p >> 3) * 10 + (p & 7)) * ORI_HP + c4;             // (ky, kx) in padded coordinates of tap q = (0, 0)
        *reinterpret_cast<f32x4*>(&act[pbase[i] + 11 * ORI_HP]) = v[i];  // interior pixel (py + 1, px + 1)
    }
    ori_head_reduce<TM>(w, pbase, part, act, wave, lane);
}

#define CNN_STAMP(k)                                                                                     \
    do {                                                                                                 \
        if (STAMPS && a.dbg_time && lane == 0) a.dbg_time[((size_t)pidx * NW + wave) * 32 + (k)] = __builtin_readcyclecounter(); \
    } while (0)

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

// What trunk form S3 (TRUNK_*, common.h) of net KIND runs in which way: the one place that reads the form's value.  The one exact OriNet instantiation has the Winograd
// and the polyphase layers (no run-time switch: the fused and the staged path both run this kernel and are pinned to each other bit for bit).
template <int KIND, int S3>
struct TrunkTraits {
    static_assert(S3 == TRUNK_EXACT || S3 == TRUNK_SPLIT2 || S3 == TRUNK_SPLIT3 || (S3 == TRUNK_WINO && KIND != AFFNET_NET_ORINET) ||
                  ((S3 == TRUNK_WINO_F43 || S3 == TRUNK_WINO_F43_C5 || S3 == TRUNK_WINO_F43_C1) && KIND == AFFNET_NET_HARDNET) || (S3 == TRUNK_WINO_POLY && KIND == AFFNET_NET_AFFNET), "no such trunk form of this net (common.h: TRUNK_*)");
    static constexpr bool EXACT = S3 != TRUNK_SPLIT2 && S3 != TRUNK_SPLIT3;     // fp32 operands on v_mfma_f32_16x16x4_f32
    // 16-channel trunks: conv1 / conv3 / conv5 as Winograd F(2x2, 3x3) on 128 registers (conv5: a wave pair per channel block); conv2 / conv4 (stride 2) as polyphase Winograd F(2x2, 2x2)
    static constexpr bool WINO13 = (S3 == TRUNK_EXACT && KIND == AFFNET_NET_ORINET) || ((S3 == TRUNK_WINO || S3 == TRUNK_WINO_POLY) && KIND == AFFNET_NET_AFFNET);
    static constexpr bool POLY16 = (S3 == TRUNK_EXACT && KIND == AFFNET_NET_ORINET) || (S3 == TRUNK_WINO_POLY && KIND == AFFNET_NET_AFFNET);
    // HardNet descriptor forms 1 / 2: conv2 / conv4 (stride 2) as polyphase Winograd F(2x2, 2x2); form 2: conv3 as Winograd F(4x4, 3x3), V shared through LDS (conv1 in F(4x4, 3x3): form 4 below)
    // form 3 (CUT5): form 2 up to conv4's loop; conv4's tensor goes to HBM and hardnet_conv5_f43_kernel (hardnet_conv5_f43.hip) runs conv5 for four patches per workgroup
    // form 4 (STREAM1): form 3 with conv0 + conv1 streamed over conv1's K, conv1 as Winograd F(4x4, 3x3) (cnn_mfma.h: F43C1L); implies CUT5, F43_3 and POLY
    static constexpr bool STREAM1 = S3 == TRUNK_WINO_F43_C1 && KIND == AFFNET_NET_HARDNET;
    static constexpr bool CUT5 = (S3 == TRUNK_WINO_F43_C5 || STREAM1) && KIND == AFFNET_NET_HARDNET;
    static constexpr bool POLY = (S3 == TRUNK_WINO || S3 == TRUNK_WINO_F43 || CUT5) && KIND == AFFNET_NET_HARDNET, F43_3 = (S3 == TRUNK_WINO_F43 || CUT5) && KIND == AFFNET_NET_HARDNET;
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

// One workgroup = one patch through one trunk.  KIND: 0 AffNet, 1 OriNet, 2 HardNet (CB = 16 / 16 / 32); NW = 8 wavefronts; S3 = the trunk form (TRUNK_*, common.h;
// TrunkTraits above says what each does - for the split-operand forms the value is the number of terms).  After the prologue that all flows share (counters, lazy skip, priority, conv0 weights, input phase) the
// kernel is one straight-line body per flow, four in all: exact HardNet (forms 0 / 1 / 2 / 3 / 4: Winograd, with polyphase conv2 / conv4 in forms 1 .. 4, conv3 in F(4x4, 3x3) in forms 2 .. 4, the body cut behind conv4 in forms 3 / 4, and conv0 + conv1 streamed with conv1 in F(4x4, 3x3) in form 4), exact AffNet / OriNet, split HardNet,
// split AffNet / OriNet; what a form or net of a flow does differently is an `if constexpr` inside that body (functions per flow or phase move registers: profiles/trunk_bodies_report.md).  Every
// layer: MFMA loop -> request the next layer's first weight chunk and bias -> barrier (all waves done reading the input) -> zero the halo of
// the OUTPUT layout, bias + ReLU + store in place -> barrier.  No HBM traffic between layers.
// AffNet / OriNet: 79 KB LDS -> 2 workgroups per CU (4 waves / SIMD, 128 VGPRs); HardNet: 154 KB LDS -> 1 workgroup per
// CU (2 waves / SIMD, 256 VGPRs).
// STAMPS = debug instantiation: the s_memtime phase stamps of tools/cnn_phase_timing.py and the per-layer activation dumps
// of affnet_cnn32_debug_layer exist only there (26 stamp sites = 26 predicated stores + branches in every wave otherwise).
template <int KIND, int NW, bool STAMPS, int S3 = 0>
__global__ __launch_bounds__(NW * 64, (KIND == AFFNET_NET_HARDNET) ? NW / 4 : 4) void cnn32_trunk_kernel(CnnArgs a, PyrSrc ps) {
    using F = TrunkTraits<KIND, S3>;
    constexpr bool EXACT = F::EXACT, WINO13 = F::WINO13, POLY16 = F::POLY16, POLY = F::POLY, F43_3 = F::F43_3, CUT5 = F::CUT5, STREAM1 = F::STREAM1;
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
        if (a.shape_op == 1) { c[CNT_SURVIVED] = 0; c[CNT_SURVIVED1] = 0; c[CNT_AFF_EVAL] = 0; c[CNT_AFF_REEVAL] = 0; }
        else if (a.shape_op == 2) c[CNT_SURVIVED1] = c[CNT_SURVIVED];
    }
    if (prow >= n || lazy_skip(a.skip_cnt, a.skip_n, blockIdx.y, CNT_SURVIVED)) return;
    const size_t pidx = (size_t)blockIdx.y * a.n_max + prow;
    if (KIND == AFFNET_NET_AFFNET && a.reeval && a.reeval[pidx] == 0) return;      // shape form 1: the margin rule left the Winograd trunk's partials of this row in place
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
    f32x4 Ur[4];                                                      // exact OriNet, Winograd AffNet: the rolling U register set of conv1 / conv3 / conv5
    if constexpr (S3 == TRUNK_EXACT && KIND == AFFNET_NET_AFFNET) prefetch_b0<NW, CB, 32, S::T1M, S::T1N, 1>(a.packed + a.off.w[1], b1, wave, lane);
    if constexpr (WINO13) wino_prefetch_u_row<NW, CB, CB, 32, Wino16::NB1>(a.wino_u, Ur, wave, lane);

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
    if constexpr (STREAM1) zero_halo<LayS1, NTHR>(act, 16);                        // the halo of the flow's conv0 output layout (form 4: of one channel block, written once for both)
    else if constexpr (EXACT) zero_halo<LayC0, NTHR>(act, CB);
    else if constexpr (S3 == TRUNK_SPLIT2) zero_halo_q<typename SplitLays<CB>::LR0, NTHR>(act);
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
    if constexpr (EXACT && KIND == AFFNET_NET_HARDNET) {
        // Exact HardNet, both descriptor forms: conv1, conv3 and conv5 (stride 1) as Winograd F(2x2, 3x3) (cnn_mfma.h) - 4/9 of the MFMAs; each wave runs NB (tile block,
        // channel block) passes of a layer, in conv1 / conv3 two at a time on one window transform (conv3x3_wino_mfma_pair_rows).  The Winograd layers
        // load their transformed weights U from the blob (NetLayout::w_wino), ahead of their use; the first fragments of a layer are requested in front of
        // the barrier before it, where the direct-form layers (conv0; form 0: conv2, conv4) request their first weight chunk.  conv5's tensor goes to HBM for
        // the head GEMM.
        // Form 1 (POLY): conv2 and conv4 (stride 2) as polyphase Winograd F(2x2, 2x2) (cnn_mfma.h: conv3x3_poly_mfma_rows) -
        // 25/36 of their MFMAs; a wave runs one unit per layer: in conv2 a tile block against a pair of channel blocks, in conv4 the one tile block against its own
        // channel block.  Their transformed weights come from a.wino_u (Poly32), which derive_u_kernel fills from the blob's taps in front of the launch; the first
        // fragments are requested in front of the barrier before the layer.  conv0, conv1, conv3, conv5 and every epilogue are the same statements for both forms.
        // Form 2 (F43_3) = form 1 with conv3 as Winograd F(4x4, 3x3) (cnn_mfma.h: conv3x3_f43_mfma_shared_v, f43_combine) - 288 instead of 512 MFMAs per wave; its
        // weights lie behind the polyphase ones at a.wino_u + F43::BASE.  conv1 runs as F(4x4, 3x3) in form 4 only (the STREAM1 block below); its U is derived in every form from 2 on.
        constexpr int T1M = S::T1M, T1N = S::T1N, T2M = S::T2M, T2N = S::T2N, T4M = S::T4M, T4N = S::T4N;
        constexpr int NB1 = (16 * 16 / 16) * (CB / 16) / NW, NB3 = (8 * 8 / 16) * (2 * CB / 16) / NW, NB5 = (4 * 4 / 16) * (4 * CB / 16) / NW;
        constexpr int NBP2 = (8 * 8 / 16) * (2 * CB / 16) / NW, NBP4 = (4 * 4 / 16) * (4 * CB / 16) / NW;      // polyphase passes per wave: conv2 a pair, conv4 one

        // ---- conv0: 1 -> CB, K = 9 (padded to 12), MFMA; reads `patch`, writes `act`: no barrier in between ----
        f32x4 Up[2][4];                                               // the rolling U register set of conv1 / conv3: one position row, both channel blocks of a pair
        f32x4 Uw[16];                                                 // the rolling U register set of conv5
        f32x4 Uf[18];                                                 // form 2: the rolling U register set of conv3
        f32x4 b2[S::G2][T2N];                                         // form 0: conv2's first weight chunk and bias
        f32x4 bias2[T2N];
        f32x4 P2a[2][3], P2b[2][3];                                   // form 1: the two rolling U register sets of conv2
        if constexpr (STREAM1) {
            // ---- form 4: conv0 + conv1 streamed over conv1's K (cnn_mfma.h: F43C1L) ---------------------------------------------
            // Per K group G of conv1: conv0 of channel block G (f43c1_conv0_tile: conv0_mfma's chain, so every conv0 value keeps the bits it has in the other forms) into the half-size
            // layout LayS1; per quarter jh of the group: every thread transforms one channel of one window into V beside it, barrier, the wave's 36 positions x 2 k-steps.
            // Wave w = (tile block w >> 1, channel block w & 1); every accumulator receives its MFMAs in the order G ascending, k-step ascending.  Stamps (the slots of the
            // phases this form does not have): 19 conv0 of G = 0 and its barrier, 20 the first quarter's transform and barrier, 2 its loop, 3 the last quarter's loop,
            // 21 output transform and barrier, 22 halo and stores, 4 barrier.
            static_assert(NW == 8 && CB == 32 && T1M == 8 && F43C1L::TOTAL <= TrunkLds<CB>::ACT, "four tile blocks x two channel blocks; conv0's half and a quarter's V fit the activation buffer");
            constexpr int DU = 6, DV = 12;                            // rolling register sets: U (L2) 6 positions = 12 MFMAs ahead - it stays live across conv0 and the transforms, and 12 spills -, V (LDS) 12 positions
            const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(a.wino_u + F43::BASE + F43::offset(1), F43_XI * CB * CB);
            const int u_lane = ((lane >> 4) * CB + (wave & 1) * 16 + (lane & 15)) * 16;
            f32x2 Ur[DU];
#pragma unroll
            for (int k = 0; k < DU; ++k) Ur[k] = f43c1_load_u<CB, CB>(wrsrc, u_lane, k, 0);
            // the transform's thread: channel 4 kq + 2 jh + j of the K group, window (ty, tx) = (wave, lane >> 3); a 32-lane half = (j, kq, tx & 3)
            const int tj = lane & 1, tkq = (lane >> 1) & 3, ttx = lane >> 3;
            const float* t_in = act + tkq * F43C1L::GS + (4 * wave * LayS1::WP + 4 * ttx) * 4 + tj;
            float* t_v = act + F43C1L::V + (wave >> 1) * 128 + F43C1L::slot(tkq, (wave & 1) * 8 + ttx) * 2 + tj;
            unsigned v0 = lds_byte_addr(act + F43C1L::V + (wave >> 1) * 128 + F43C1L::slot(lane >> 4, lane & 15) * 2), v1 = v0 + 18 * F43C1L::XS * 4;
            asm("" : "+v"(v0));
            asm("" : "+v"(v1));
            f32x4 acc[F43_XI];
#pragma unroll
            for (int k = 0; k < F43_XI; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int G = 0; G < 2; ++G) {
                // every wave is past the previous K group's last transform (which read LayS1) since the barrier in front of that quarter's loop
                {
                    float wg[3];
#pragma unroll
                    for (int s3 = 0; s3 < 3; ++s3) wg[s3] = G ? w0[s3][1] : w0[s3][0];
                    f43c1_conv0_tile(patch, wg, G ? bias0[1] : bias0[0], act, wave, lane);
                }
                __syncthreads();                                      // conv0's channel block is in place; every wave has finished the previous quarter's loop (V is free)
                if (G == 0) CNN_STAMP(19);
#pragma unroll 1
                for (int jh = 0; jh < 2; ++jh) {
                    if (jh) __syncthreads();                          // every wave has finished the previous quarter's loop: V is free
                    f43_transform_channel<LayS1::WP, F43C1L::XS>(t_in + 2 * jh, t_v);
                    __syncthreads();                                  // V of the quarter is in place
                    if (G == 0 && jh == 0) CNN_STAMP(20);
                    const int q_off = G * (16 * CB * 4) + jh * 8, q_next = jh == 0 ? q_off + 8 : (G == 0 ? 16 * CB * 4 : q_off);
                    __builtin_amdgcn_s_setprio(0);
                    f43c1_quarter_loop<CB, CB, DU, DV>(wrsrc, u_lane, q_off, q_next, v0, v1, Ur, acc);
                    __builtin_amdgcn_s_setprio(3);
                    if (G == 0 && jh == 0) CNN_STAMP(2);
                }
            }
            CNN_STAMP(3);
            f32x4 y[16];
            f43c5_output(acc, y);
            poly_prefetch_u<NW, CB, 2 * CB, 16, NBP2, 2>(a.wino_u + Poly32::offset(2), P2a, P2b, wave, lane);
            const f32x4 bf = *reinterpret_cast<const f32x4*>(&a.packed[a.off.b[1] + (wave & 1) * 16 + 4 * (lane >> 4)]);
            __syncthreads();                                          // every wave has finished reading V
            CNN_STAMP(21);
            zero_halo<LayC1, NTHR>(act, CB);
            f43c1_store_lds<LayC1>(act, bf, y, wave, lane);
            CNN_STAMP(22);
            __syncthreads();
            CNN_STAMP(4);
        }
        if constexpr (!STREAM1) {
            f32x4 acc[T1M][T1N];
            conv0_mfma<NW, CB, T1M, T1N>(patch, w0, bias0, acc, wave, lane);
            CNN_STAMP(19);
            store_tiles_lds<CB, LayC0, T1M, T1N, false>(act, bias0, acc, wave, lane);
            CNN_STAMP(20);
            wino_prefetch_u_pair<NW, CB, CB, 32, NB1>(a.packed + a.off.w_wino[0], Up, wave, lane);
            __syncthreads();
        }
        if (!STREAM1 && STAMPS && a.dbg_layer == 0) { dump_planes<CB, LayC0, NTHR>(act, a.dbg_out); return; }
        if constexpr (!STREAM1) CNN_STAMP(2);

        // ---- conv1: CB -> CB @32x32, Winograd -------------------------------------------------------------
        if constexpr (!STREAM1) {
            f32x4 y[NB1][4], bw[NB1];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_wino_mfma_pair_rows<NW, CB, CB, LayC0, NB1>(act, a.packed + a.off.w_wino[0], Up, y, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(3);
            if constexpr (POLY) poly_prefetch_u<NW, CB, 2 * CB, 16, NBP2, 2>(a.wino_u + Poly32::offset(2), P2a, P2b, wave, lane);
            else {
                prefetch_b0<NW, 2 * CB, 16, T2M, T2N, S::G2>(a.packed + a.off.w[2], b2, wave, lane);
                prefetch_bias<NW, 16, T2M, T2N>(a.packed + a.off.b[2], bias2, wave, lane);
            }
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

        // ---- conv2: CB -> 2CB, stride 2 @16x16; form 1: polyphase --------------------------------------------
        if constexpr (POLY) {
            f32x4 y[NBP2][4], bw[NBP2];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_poly_mfma_rows<NW, CB, 2 * CB, LayC1, NBP2, 2>(act, a.wino_u + Poly32::offset(2), P2a, P2b, y, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(5);
            if constexpr (F43_3) f43_prefetch_u<2 * CB, 2 * CB>(a.wino_u + F43::BASE + F43::offset(3), Uf, wave, lane);
            else wino_prefetch_u_pair<NW, 2 * CB, 2 * CB, 16, NB3>(a.packed + a.off.w_wino[1], Up, wave, lane);
            wino_bias<NW, 16, 2 * CB, NBP2>(a.packed + a.off.b[2], bw, wave, lane);
            __syncthreads();
            zero_halo<LayC2, NTHR>(act, 2 * CB);
            wino_store_lds<2 * CB, LayC2, NBP2>(act, bw, y, wave, lane);
            __syncthreads();
            CNN_STAMP(6);
        } else {
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
        f32x4 b4[S::G4][T4N];                                         // form 0: conv4's first weight chunk and bias
        f32x4 bias4[T4N];
        f32x4 P4a[1][3], P4b[1][3];                                   // form 1: the two rolling U register sets of conv4
        if constexpr (F43_3) {
            // form 2: F(4x4, 3x3), a wave pair per channel block (cnn_mfma.h: conv3x3_f43_mfma_shared_v); stamp 7 sits behind the halves' exchange
            static_assert(F43L::V_FLOATS <= TrunkLds<CB>::ACT && F43L::X + F43L::X_FLOATS <= F43L::V_FLOATS, "conv3: V of the layer fits the activation buffer");
            f32x4 tf[3][4], y[8];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_f43_mfma_shared_v<NW, 2 * CB, 2 * CB, LayC2>(act, a.wino_u + F43::BASE + F43::offset(3), Uf, tf, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(23);
            poly_prefetch_u<NW, 2 * CB, 4 * CB, 8, NBP4, 1>(a.wino_u + Poly32::offset(4), P4a, P4b, wave, lane);
            const f32x4 bf = *reinterpret_cast<const f32x4*>(&a.packed[a.off.b[3] + (wave >> 1) * 16 + 4 * (lane >> 4)]);
            __syncthreads();                                          // every wave has finished reading V
            f43_combine(act, tf, y, wave, lane);
            CNN_STAMP(7);
            __syncthreads();                                          // ... and its partner's exchange slot
            zero_halo<LayC3, NTHR>(act, 2 * CB);
            f43_store_lds<LayC3>(act, bf, y, wave, lane);
            __syncthreads();
            CNN_STAMP(8);
        } else {
            f32x4 y[NB3][4], bw[NB3];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_wino_mfma_pair_rows<NW, 2 * CB, 2 * CB, LayC2, NB3>(act, a.packed + a.off.w_wino[1], Up, y, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(7);
            if constexpr (POLY) poly_prefetch_u<NW, 2 * CB, 4 * CB, 8, NBP4, 1>(a.wino_u + Poly32::offset(4), P4a, P4b, wave, lane);
            else {
                prefetch_b0<NW, 4 * CB, 8, T4M, T4N, S::G4>(a.packed + a.off.w[4], b4, wave, lane);
                prefetch_bias<NW, 8, T4M, T4N>(a.packed + a.off.b[4], bias4, wave, lane);
            }
            wino_bias<NW, 16, 2 * CB, NB3>(a.packed + a.off.b[3], bw, wave, lane);
            __syncthreads();
            zero_halo<LayC3, NTHR>(act, 2 * CB);
            wino_store_lds<2 * CB, LayC3, NB3>(act, bw, y, wave, lane);
            __syncthreads();
            CNN_STAMP(8);
        }
        if (STAMPS && a.dbg_layer == 3) { dump_planes<2 * CB, LayC3, NTHR>(act, a.dbg_out); return; }

        // ---- conv4: 2CB -> 4CB, stride 2 @8x8; form 1: polyphase ----------------------------------------------
        if constexpr (POLY) {
            f32x4 y[NBP4][4], bw[NBP4];
            __builtin_amdgcn_s_setprio(0);
            conv3x3_poly_mfma_rows<NW, 2 * CB, 4 * CB, LayC3, NBP4, 1>(act, a.wino_u + Poly32::offset(4), P4a, P4b, y, wave, lane);
            __builtin_amdgcn_s_setprio(3);
            CNN_STAMP(9);
            if constexpr (!CUT5) wino_prefetch_u<NW, 4 * CB, 4 * CB, 8, NB5>(a.packed + a.off.w_wino[2], Uw, wave, lane);
            wino_bias<NW, 8, 4 * CB, NBP4>(a.packed + a.off.b[4], bw, wave, lane);
            if constexpr (CUT5) {
                // form 3 ends here: bias, ReLU and conv4's tensor into the patch's slot of a.out as [c / 4][pixel][4], the LDS layout without its halo
                if (!STAMPS || a.dbg_layer < 0) {
                    wino_store_global_c4<4 * CB, 8, NBP4>(a.out + pidx * (64 * 4 * CB), bw, y, wave, lane);
                    CNN_STAMP(13);
                    return;
                }
            }
            __syncthreads();
            zero_halo<LayC4, NTHR>(act, 4 * CB);
            wino_store_lds<4 * CB, LayC4, NBP4>(act, bw, y, wave, lane);
            __syncthreads();
            CNN_STAMP(10);
        } else {
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
        if constexpr (!CUT5) {
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
        }
    } else if constexpr (EXACT) {
        // Exact AffNet / OriNet.  OriNet: conv1, conv3 and conv5 (stride 1) as Winograd F(2x2, 3x3), one row of four transform positions at a time
        // (conv3x3_wino_mfma_rows: the 128-register budget of two workgroups per CU) - 4/9 of their MFMAs; U = G g G^T comes from a.wino_u, which
        // derive_u_kernel fills from the blob's taps in front of every launch.  AffNet, S3 = 0: conv1 .. conv5 in the direct form; S3 = 1: conv1 / conv3 / conv5 as
        // OriNet runs them.  AffNet's output decides the shape filter, whose eigenvalue test (shape_filter.h: d1 = tr^2 - 4 det > 0) turns on the LAST
        // bits of A for near-isotropic shapes, so another rounding alone changes which keypoints a call returns (measured: 124 of 128 000 ids at the headline
        // configuration): the rows where it could are recomputed by the S3 = 0 kernel (a.reeval).  conv0 (and the S3 = 0 kernel's conv5) in the direct form; conv2 / conv4
        // (stride 2) direct as well, or - POLY16: the exact OriNet kernel and AffNet's S3 = 5 - as polyphase Winograd F(2x2, 2x2) (cnn_mfma.h: conv3x3_poly16_mfma_rows; U behind the
        // Winograd sections of a.wino_u); conv5 straight into the heads (AffNet from the direct form's accumulators or, S3 = 1, from the Winograd fragments; OriNet from its Winograd fragments through an LDS copy).
        constexpr int T1M = S::T1M, T1N = S::T1N, T2M = S::T2M, T2N = S::T2N, T4M = S::T4M, T4N = S::T4N;
        static_assert(NW == 8 && CB == 16, "Wino16 describes the 16-channel trunks on 8 waves");
        constexpr int NB1 = Wino16::NB1, NB3 = Wino16::NB3;
        static_assert(WINO13 || T1M * 8 > S::AREG, "conv1: two A sets of T1M float4 do not fit -> rolling single set (conv3x3_mfma_roll)");
        f32x4 b4[S::G4][T4N];
        f32x4 bias4[T4N];
        f32x4 bias1[T1N];                                             // the direct form's conv1 / conv3 (!WINO13): conv1's bias, conv3's first weight chunk and bias
        f32x4 b3[S::G3][T2N];
        f32x4 bias3[T2N];
        f32x4 Upa[3], Upb[3];                                         // POLY16: the two rolling U register sets of conv2 / conv4
        static_assert(!POLY16 || WINO13, "the polyphase stride-2 layers sit between the Winograd stride-1 layers");
        // ---- conv0: 1 -> CB, K = 9 (padded to 12), MFMA; reads `patch`, writes `act`: no barrier in between ----
        {
            f32x4 acc[T1M][T1N];
            conv0_mfma<NW, CB, T1M, T1N>(patch, w0, bias0, acc, wave, lane);
            CNN_STAMP(19);
            if constexpr (!WINO13) prefetch_bias<NW, 32, T1M, T1N>(a.packed + a.off.b[1], bias1, wave, lane);
            store_tiles_lds<CB, LayC0, T1M, T1N, false>(act, bias0, acc, wave, lane);
            CNN_STAMP(20);
            __syncthreads();
        }
        if (STAMPS && a.dbg_layer == 0) { dump_planes<CB, LayC0, NTHR>(act, a.dbg_out); return; }
        CNN_STAMP(2);

        // ---- conv1: CB -> CB @32x32, Winograd or direct ------------------------------------------------------
        f32x4 b2[S::G2][T2N];
        f32x4 bias2[T2N];
        if constexpr (WINO13) {
            f32x4 y[NB1][4], bw[NB1];
            conv3x3_wino_mfma_rows<NW, CB, CB, LayC0, NB1>(act, a.wino_u, Ur, y, wave, lane);
            CNN_STAMP(3);
            if constexpr (POLY16) poly16_prefetch_u<CB, 2 * CB>(a.wino_u + Wino16::offset(2), Upa, Upb, wave & 1, 0, lane);
            else {
                prefetch_b0<NW, 2 * CB, 16, T2M, T2N, S::G2>(a.packed + a.off.w[2], b2, wave, lane);
                prefetch_bias<NW, 16, T2M, T2N>(a.packed + a.off.b[2], bias2, wave, lane);
            }
            wino_bias<NW, 32, CB, NB1>(a.packed + a.off.b[1], bw, wave, lane);
            __syncthreads();
            CNN_STAMP(21);
            zero_halo<LayC1, NTHR>(act, CB);
            wino_store_lds<CB, LayC1, NB1>(act, bw, y, wave, lane);
            CNN_STAMP(22);
            __syncthreads();
            CNN_STAMP(4);
        } else {
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

        // ---- conv2: CB -> 2CB, stride 2 @16x16; POLY16: polyphase, one (tile block, channel block) unit per wave --------
        if constexpr (POLY16) {
            f32x4 y[1][4], bw[1];
            int ty, tx, cb;
            wino_tile<16, 2 * CB, 1>(wave, 0, lane & 15, ty, tx, cb);
            static_assert((16 / 2) * (16 / 2) / 16 * (2 * CB / 16) == NW, "conv2: one unit per wave");
            conv3x3_poly16_mfma_rows<CB, 2 * CB, LayC1>(act, a.wino_u + Wino16::offset(2), Upa, Upb, y[0], ty, tx, cb, 0, lane);
            CNN_STAMP(5);
            wino_prefetch_u_row<NW, 2 * CB, 2 * CB, 16, NB3>(a.wino_u + Wino16::offset(3), Ur, wave, lane);
            wino_bias<NW, 16, 2 * CB, 1>(a.packed + a.off.b[2], bw, wave, lane);
            __syncthreads();
            zero_halo<LayC2, NTHR>(act, 2 * CB);
            wino_store_lds<2 * CB, LayC2, 1>(act, bw, y, wave, lane);
            __syncthreads();
            CNN_STAMP(6);
        } else {
            f32x4 acc[T2M][T2N];
            conv3x3_mfma<NW, CB, 2 * CB, LayC1, 2, T2M, T2N, S::G2>(act, a.packed + a.off.w[2], b2, acc, wave, lane);
            CNN_STAMP(5);
            if constexpr (WINO13) wino_prefetch_u_row<NW, 2 * CB, 2 * CB, 16, NB3>(a.wino_u + Wino16::offset(3), Ur, wave, lane);
            else {
                prefetch_b0<NW, 2 * CB, 16, T2M, T2N, S::G3>(a.packed + a.off.w[3], b3, wave, lane);
                prefetch_bias<NW, 16, T2M, T2N>(a.packed + a.off.b[3], bias3, wave, lane);
            }
            __syncthreads();
            zero_halo<LayC2, NTHR>(act, 2 * CB);
            store_tiles_lds<2 * CB, LayC2, T2M, T2N>(act, bias2, acc, wave, lane);
            __syncthreads();
            CNN_STAMP(6);
        }
        if (STAMPS && a.dbg_layer == 2) { dump_planes<2 * CB, LayC2, NTHR>(act, a.dbg_out); return; }

        // ---- conv3: 2CB -> 2CB @16x16, Winograd or direct ----------------------------------------------------
        if constexpr (WINO13) {
            f32x4 y[NB3][4], bw[NB3];
            conv3x3_wino_mfma_rows<NW, 2 * CB, 2 * CB, LayC2, NB3>(act, a.wino_u + Wino16::offset(3), Ur, y, wave, lane);
            CNN_STAMP(7);
            if constexpr (POLY16) poly16_prefetch_u<2 * CB, 4 * CB>(a.wino_u + Wino16::offset(4), Upa, Upb, wave >> 1, wave & 1, lane);
            else {
                prefetch_b0<NW, 4 * CB, 8, T4M, T4N, S::G4>(a.packed + a.off.w[4], b4, wave, lane);
                prefetch_bias<NW, 8, T4M, T4N>(a.packed + a.off.b[4], bias4, wave, lane);
            }
            wino_bias<NW, 16, 2 * CB, NB3>(a.packed + a.off.b[3], bw, wave, lane);
            __syncthreads();
            zero_halo<LayC3, NTHR>(act, 2 * CB);
            wino_store_lds<2 * CB, LayC3, NB3>(act, bw, y, wave, lane);
            __syncthreads();
            CNN_STAMP(8);
        } else {
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

        // ---- conv4: 2CB -> 4CB, stride 2 @8x8 --------------------------------------------------------------
        f32x4 b5[S::G5][T4N];
        f32x4 bias5[T4N];
        if constexpr (POLY16) {
            // POLY16: polyphase; wave 2 p + h runs channel block p on K group h, the pair adds its partial y through LDS (cnn_mfma.h: poly16_combine); stamp 9 sits behind the exchange
            static_assert(Poly16::X >= (2 * CB / 4) * LayC3::PSG && Poly16::X + Poly16::X_FLOATS <= TrunkLds<CB>::TOTAL && (4 * CB / 4) * LayC4::PSG <= Poly16::X,
                          "polyphase conv4: the exchange lies behind conv3's output inside the LDS array, and conv4's output in front of the exchange");
            f32x4 y[4], yo[2];
            conv3x3_poly16_mfma_rows<2 * CB, 4 * CB, LayC3>(act, a.wino_u + Wino16::offset(4), Upa, Upb, y, (lane & 15) >> 2, lane & 3, wave >> 1, wave & 1, lane);
            CNN_STAMP(24);
            wino5_prefetch_u(a.wino_u + Wino16::offset(5), Ur, wave, lane);
            const f32x4 bw = *reinterpret_cast<const f32x4*>(&a.packed[a.off.b[4] + (wave >> 1) * 16 + 4 * (lane >> 4)]);
            poly16_combine(lds, y, yo, wave, lane);
            CNN_STAMP(9);
            zero_halo<LayC4, NTHR>(act, 4 * CB);
            wino5_store_lds<LayC4::WP, 4, LayC4::PSG>(act + (LayC4::WP + 1) * 4, bw, yo, wave, lane);
            __syncthreads();
            CNN_STAMP(10);
        } else {
            f32x4 acc[T4M][T4N];
            conv3x3_mfma<NW, 2 * CB, 4 * CB, LayC3, 2, T4M, T4N, S::G4>(act, a.packed + a.off.w[4], b4, acc, wave, lane);
            CNN_STAMP(9);
            if constexpr (WINO13) {
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

        static_assert(!WINO13 || (Wino5::X >= 16 * LayC4::PSG && Wino5::X + Wino5::X_FLOATS <= TrunkLds<CB>::TOTAL),
                      "Winograd conv5: the exchange lies behind conv4's output inside the LDS array");
        if constexpr (WINO13) {
            // ---- conv5: 4CB -> 4CB @8x8, Winograd, a wave pair per channel block (the loop below, then wino5_combine), then the head's per-wave partial sums.
            // OriNet: the 2 x 2-pixel fragments go into the head's 10 x 10 copy (over conv4's output, which is dead by then).  AffNet's Winograd form: straight from the
            // combined fragments (head_partials_wino: no LDS copy, no barrier beyond the combine's).  Both request the head's weights in front of the combine's barrier ----
            constexpr bool ORI = KIND == AFFNET_NET_ORINET;
            static_assert(T4M == 2, "hw: one weight vector per (output, pixel tile) for OriNet, per (output, fragment pixel) for AffNet");
            static_assert(!ORI || Wino5::HEAD + 100 * ORI_HP <= Wino5::X, "conv5: the head copy in front of the exchange");
            f32x4 acc[2][4], y[2], hw[ORI ? 2 : 3][2];
            conv3x3_wino_mfma_half_rows<NW, LayC4>(act, a.wino_u + Wino16::offset(5), Ur, acc, wave, lane);
            CNN_STAMP(11);
            const f32x4 bw = *reinterpret_cast<const f32x4*>(&a.packed[a.off.b[5] + (wave >> 1) * 16 + 4 * (lane >> 4)]);
            const OriHeadLane HL = OriHeadLane::of<T4M>(wave, lane);
            if (!STAMPS || a.dbg_layer < 0) {
                if constexpr (ORI) ori_head_weights<T4M>(a.packed + a.off.head_w, HL, hw);
                else aff_head_weights_wino(a.packed + a.off.head_w, hw, wave, lane);
            }
            wino5_combine(lds, acc, y, wave, lane);
            if (!STAMPS || a.dbg_layer < 0) {
                if constexpr (ORI) {
                    float* copy = lds + Wino5::HEAD;
                    ori_head_zero_halo<NTHR>(copy, tid);
                    wino5_store_lds<10, ORI_HP, 4>(copy + 11 * ORI_HP, bw, y, wave, lane);
                    int pbase[T4M];
                    ori_head_pbase<T4M>(HL, pbase);
                    ori_head_reduce<T4M>(hw, pbase, a.out + pidx * HEAD_PART_ORI, copy, wave, lane);
                } else {
                    head_partials_wino(hw, bw, y, a.out + pidx * HEAD_PART_AFF, wave, lane);
                }
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

// The getter of a cnn_trunk_*.hip unit: instantiates net KIND in FORMS..., product and stamped, and returns the one asked for; NULL for a form that is not among them
template <int KIND, int... FORMS>
TrunkKernel trunk_unit(int form, bool stamps) {
    TrunkKernel k = nullptr;
    ((form == FORMS ? (void)(k = !stamps ? cnn32_trunk_kernel<KIND, 8, false, FORMS> : cnn32_trunk_kernel<KIND, 8, true, FORMS>) : (void)0), ...);
    return k;
}
