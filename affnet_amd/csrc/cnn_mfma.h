// Shared MFMA building blocks of the 32x32-patch trunks (cnn_trunk.h), their heads (cnn_heads.hip) and the fully-convolutional AffNet (fullconv.hip):
// LDS activation layouts, weight fragment loads, the software-pipelined implicit-GEMM 3x3 convolution on
// v_mfma_f32_16x16x4_f32, conv0 on the matrix cores and the tile epilogues.  gfx950 only.  The packed weight blob these loops read -
// sections, offsets and element orders - is defined in weights_layout.h (included here) and filled by weights_pack.hip.
#pragma once
#include <math.h>
#include <stdlib.h>

#include <utility>

#include "common.h"
#include "weights_layout.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// LDS activation layout: channel-interleaved by 4.  A tensor [C][H][H] lives as C/4 "plane groups"; element
// (c, y, x) of the zero-haloed (H+2)-square image sits at  (c/4)*PSG + ((y+1)*WP + x+1)*4 + c%4  (floats).  One
// ds_read_b128 of lane (pixel m, kq) then delivers the A operands of FOUR MFMA k-steps (channels 4*(4G+kq)+j,
// j = 0..3) - a quarter of the LDS instructions and half the LDS cycles of per-k-step ds_read_b32, which is what
// kept the matrix pipe waiting: under 16-32 waves of MFMA loops an LDS read returns after several hundred cycles and
// lgkmcnt (4 bits) cannot cover more than 15 reads in flight.  The packed weights are interleaved the same way, so a
// B fragment is one coalesced global_load_dwordx4 per 4 k-steps (1 KB per wave instruction).
//
// Each buffer is written by one layer's epilogue and read by the next layer's implicit GEMM; (WP, PSG) are chosen for
// the READER (ds_read_b128 services lanes {0-3,12-15,20-27},{4-11,16-19,28-31},... per cycle over 64 banks):
//   stride-1 reader: 16 consecutive pixels = 64 banks; the kq = 1 lanes of a group must land on the other half:
//                    H = 32/16: PSG == 0 (mod 64);  H = 8 (a tile = 2 rows): WP = 16, PSG == 32 (mod 64);
//   stride-2 reader: pixels 2 apart hit banks == 0..3 (mod 8) -> PSG == 4 (mod 8) (and WP == 0 (mod 8) when a tile
//                    spans two output rows, 16 -> 8) - these also make the epilogue's ds_write_b32 conflict free.
//
// Operand roles: the WEIGHTS are the MFMA "A" operand (rows = 16 output channels) and the ACTIVATIONS the "B" operand
// (columns = 16 pixels), i.e. each 16x16 tile is out^T[channel][pixel].  A lane then owns FOUR CONSECUTIVE CHANNELS of one
// pixel (rows 4g..4g+3 of column lane&15) = exactly one float4 of the interleaved layout, so the epilogue is one
// conflict-free ds_write_b128 per tile instead of four 4-way-conflicting ds_write_b32.
// LDS reads of the MFMA loops go through an explicit 32-bit LDS byte address: one address VGPR per K group (made
// opaque to the optimiser) + a compile-time immediate per tile.  Left to itself the compiler folds the chunk constant
// into every tile offset, overflows the 16-bit DS offset field and spends one v_add_u32 per ds_read_b128 inside the
// MFMA stream (conv1: 8 per 64 MFMAs, -12 % MFMA rate in tools/mfma_probe.py).
typedef __attribute__((address_space(3))) const f32x4 LdsF4;
__device__ __forceinline__ unsigned lds_byte_addr(const float* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const float*)p;
}
__device__ __forceinline__ f32x4 lds_read4(unsigned byte_addr) { return *(LdsF4*)(size_t)byte_addr; }

// Weight fragments of the MFMA loops come through a buffer descriptor: the lane offset is one loop-invariant 32-bit
// VGPR, the chunk offset an SGPR, the tile offset an immediate - no 64-bit VALU pointer arithmetic between the MFMAs and
// half the address payload of a flat global_load_dwordx4 per instruction.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t weight_rsrc(const float* base, int n_floats) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, n_floats * 4, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_read4(__amdgpu_buffer_rsrc_t r, int lane_byte_off, int uniform_byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, lane_byte_off, uniform_byte_off, 0));
}

template <int H_, int WP_, int PSG_>
struct Lay {
    static constexpr int H = H_, WP = WP_, PSG = PSG_;
    __device__ static __forceinline__ int at(int c, int y, int x) { return (c >> 2) * PSG + ((y + 1) * WP + x + 1) * 4 + (c & 3); }
};
typedef Lay<32, 34, 4672> LayC0;   // conv0 out -> conv1 (stride 1)
typedef Lay<32, 34, 4628> LayC1;   // conv1 out -> conv2 (stride 2)
typedef Lay<16, 18, 1344> LayC2;   // conv2 out -> conv3 (stride 1)
typedef Lay<16, 24, 1732> LayC3;   // conv3 out -> conv4 (stride 2, tile = 2 output rows)
typedef Lay<8, 16, 672> LayC4;     // conv4 out -> conv5 (stride 1, tile = 2 rows)
typedef Lay<8, 16, 672> LayC5;     // conv5 out -> AffNet / OriNet heads
#define WP32 34

// ---- device helpers ------------------------------------------------------------------------------
// Wave-wide sum on the VALU only (DPP row reductions + 4 readlanes).  __shfl_xor compiles to ds_bpermute_b32,
// i.e. six DEPENDENT trips through the LDS queue, which the MFMA loops of the co-resident waves keep hundreds of
// requests deep: the two input-norm reductions cost ~15k cycles per patch that way (profiles/r01_s2b_cnn_phase_timing).
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum(float v) {
    v = dpp_add<0xB1>(v);     // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);     // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);    // row_half_mirror: 8 lanes
    v = dpp_add<0x140>(v);    // row_mirror: every lane holds the sum of its row of 16
    const int iv = __float_as_int(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(iv, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(iv, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(iv, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(iv, 48));
    return (r0 + r1) + (r2 + r3);
}

// Sum `v` over the NW wavefronts of the workgroup.  `slot` must hold NW floats that nothing else touches during the
// kernel (each reduction of a kernel gets its own slot), so ONE barrier suffices.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* slot) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += slot[w];
    return t;
}

// Zero the 1-pixel halo of the C/4 plane groups of layout L (16-byte stores).
template <typename L, int NTHR>
__device__ __forceinline__ void zero_halo(float* act, int channels, int tid = threadIdx.x) {
    constexpr int H = L::H, CELLS = 4 * (H + 1);
    const int groups = channels >> 2;
    for (int i = tid; i < groups * CELLS; i += NTHR) {
        const int g = i / CELLS, e = i - g * CELLS;
        int y, x;
        if (e < H + 2) { y = 0; x = e; }
        else if (e < 2 * (H + 2)) { y = H + 1; x = e - (H + 2); }
        else { const int r = e - 2 * (H + 2); y = 1 + (r >> 1); x = (r & 1) ? H + 1 : 0; }
        *reinterpret_cast<f32x4*>(&act[g * L::PSG + (y * L::WP + x) * 4]) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
}

// Plane groups (16 input channels = 4 MFMA k-steps) per pipeline chunk: grow the chunk until it holds `target`
// MFMAs, as long as the two A register sets stay within `max_a_regs` VGPRs.
constexpr int pick_groups(int cin, int tm, int tn, int target, int max_a_regs) {
    int g = 1;
    while (g * 2 <= cin / 16 && (cin / 16) % (g * 2) == 0 && 4 * tm * tn * g < target && 2 * (g * 2) * tm * 4 <= max_a_regs) g *= 2;
    return g;
}

// Implicit-GEMM 3x3 convolution (padding 1) of the LDS tensor `act` (layout LI, CIN channels) with packed weights
// Wg [tap][CIN/16][kq][COUT][4]; leaves the TM x TN tiles (16 px x 16 ch) of this wave in `acc` (pre-activation, no
// bias).  HOUT = LI::H / STRIDE.  K is walked in chunks of GRP plane groups (a chunk never straddles a tap).
// Software pipeline, one chunk deep, two statically named register sets: while the MFMAs of chunk c issue, the A
// (ds_read_b128) and B (global_load_dwordx4) fragments of chunk c+1 are in flight; loads and MFMAs interleave per
// plane group so that few LDS reads are outstanding at any wait (lgkmcnt has 4 bits).
template <int GRP, int TM, int TN>
struct Frag {
    f32x4 a[GRP][TM];
    f32x4 b[GRP][TN];
};

// B fragments of chunk 0 of a layer (and its bias values): they do not depend on the activations, so the kernel requests
// them BEFORE the barriers / epilogue of the previous layer and their L2 latency (1-2k cycles under load) is hidden.
template <int NW, int COUT, int HOUT, int TM, int TN, int GRP>
__device__ __forceinline__ void prefetch_b0(const float* __restrict__ Wg, f32x4 (&b0)[GRP][TN], int wave, int lane) {
    constexpr int MG = (HOUT * HOUT / 16) / TM;
    const int ng = wave / MG, m = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int u = 0; u < GRP; ++u)
#pragma unroll
        for (int j = 0; j < TN; ++j) b0[u][j] = *reinterpret_cast<const f32x4*>(&Wg[u * 16 * COUT + (kq * COUT + (ng * TN + j) * 16 + m) * 4]);
}
template <int NW, int HOUT, int TM, int TN>
__device__ __forceinline__ void prefetch_bias(const float* __restrict__ bias, f32x4 (&bv)[TN], int wave, int lane) {
    constexpr int MG = (HOUT * HOUT / 16) / TM;
    const int ng = wave / MG;
#pragma unroll
    for (int j = 0; j < TN; ++j) bv[j] = *reinterpret_cast<const f32x4*>(&bias[(ng * TN + j) * 16 + 4 * (lane >> 4)]);   // channels 4g..4g+3
}

// Same with the lane index made opaque: the compiler then recomputes 4 * (lane >> 4) here instead of keeping it in a register across the
// whole kernel (at the 128-VGPR cap of the 16-channel split trunks that one value was spilled to scratch).
template <int NW, int HOUT, int TM, int TN>
__device__ __forceinline__ void prefetch_bias_fresh(const float* __restrict__ bias, f32x4 (&bv)[TN], int wave, int lane) {
    asm volatile("" : "+v"(lane));
    prefetch_bias<NW, HOUT, TM, TN>(bias, bv, wave, lane);
}

// PROBE (tuning aid, affnet_cnn32_probe): bit 0 = skip the weight loads, bit 1 = skip the activation loads inside the loop,
// bit 3 = activation reads from lane-consecutive addresses (bank-conflict-free reference pattern).
template <int NW, int CIN, int COUT, typename LI, int STRIDE, int TM, int TN, int GRP, int PROBE = 0>
__device__ __forceinline__ void conv3x3_mfma(const float* act, const float* __restrict__ Wg, const f32x4 (&b0)[GRP][TN],
                                             f32x4 (&acc)[TM][TN], int wave, int lane) {
    constexpr int HOUT = LI::H / STRIDE;
    constexpr int MT = HOUT * HOUT / 16, NT = COUT / 16;
    constexpr int MG = MT / TM, NG = NT / TN;
    constexpr int NGRP = CIN / 16, NCHUNK = 9 * NGRP / GRP;
    static_assert(MG * NG == NW, "the waves must tile the layer exactly");
    static_assert(CIN % 16 == 0 && NGRP % GRP == 0, "bad chunking");
    const int mg = wave % MG, ng = wave / MG;
    const int m = lane & 15, kq = lane >> 4;
    // lane address of tile 0 / N-tile 0; the other tiles of the wave sit at compile-time offsets (immediates)
    static_assert(HOUT == 8 || (TM * 16) % HOUT == 0 || HOUT % (TM * 16) == 0, "tile offsets must be wave-uniform constants");
    int a_lane;
    {
        const int p = mg * TM * 16 + m;
        const int oy = p / HOUT, ox = p - oy * HOUT;
        a_lane = kq * LI::PSG + ((oy * STRIDE) * LI::WP + ox * STRIDE) * 4;
    }
    const int b_lane = (kq * COUT + ng * TN * 16 + m) * 4;
    if (PROBE & 8) a_lane = lane * 4;                      // probe: 64 consecutive float4 per read = the conflict-free ideal
    const unsigned a_addr0 = lds_byte_addr(act) + a_lane * 4;
    auto a_imm = [](int i) {                               // byte offset of tile i from tile 0 (compile-time after unrolling)
        return 4 * ((PROBE & 8) ? i * 256 : (HOUT == 8 ? i * 2 * STRIDE * LI::WP * 4 : (((i * 16) / HOUT) * STRIDE * LI::WP + ((i * 16) % HOUT) * STRIDE) * 4));
    };
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    Frag<GRP, TM, TN> f0, f1;

    auto a_chunk_off = [](int ch) {
        const int q0 = ch * GRP;
        const int tap = q0 / NGRP, g0 = q0 - tap * NGRP;
        const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;          // tap / 3, tap % 3 for tap < 9
        return g0 * 4 * LI::PSG + (ky * LI::WP + kx) * 4;
    };
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wg, 9 * CIN * COUT);
    auto load_group = [&](Frag<GRP, TM, TN>& f, int u, int a_off, int w_off) {
        if (!(PROBE & 2)) {
            unsigned ab = a_addr0 + (a_off + u * 4 * LI::PSG) * 4;
            asm("" : "+v"(ab));
#pragma unroll
            for (int i = 0; i < TM; ++i) f.a[u][i] = lds_read4(ab + a_imm(i));
        }
        if (!(PROBE & 1)) {
#pragma unroll
            for (int j = 0; j < TN; ++j) f.b[u][j] = buf_read4(wrsrc, b_lane * 4 + j * 256, (w_off + u * 16 * COUT) * 4);
        }
    };
    auto mfma_group = [&](const Frag<GRP, TM, TN>& f, int u) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.b[u][j][s4], f.a[u][i][s4], acc[i][j], 0, 0, 0);   // W^T x act
    };
    // compute the chunk held in `cur` while loading chunk `nxt_ch` into `nxt`
    auto stage = [&](const Frag<GRP, TM, TN>& cur, Frag<GRP, TM, TN>& nxt, int nxt_ch) {
        const int a_off = a_chunk_off(nxt_ch);
        const int w_off = nxt_ch * (GRP * 16 * COUT);
#pragma unroll
        for (int u = 0; u < GRP; ++u) {
            load_group(nxt, u, a_off, w_off);
            mfma_group(cur, u);
            // Schedule: the TM ds_read_b128 and TN global_load_dwordx4 of this group are spread BETWEEN its MFMAs (one load
            // after every Q MFMAs) instead of being issued as a burst in front of them.  A wave cannot issue an MFMA while it
            // issues a load (a 1 KB dwordx4 wave-load holds the issue slot for tens of cycles); with bursts at the group
            // boundaries both waves of a SIMD tended to be in their bursts together and the pipe idled ~8 % of the loop
            // (tools/mfma_probe.py: conv1 81.7 % -> 88.5 % of peak with the weight loads removed).
            constexpr int NM = 4 * TM * TN, NL = ((PROBE & 2) ? 0 : TM) + ((PROBE & 1) ? 0 : TN), Q = NL ? NM / (NL + 1) : NM;
            // weight loads (L2, long latency) first, activation loads (LDS) after them
#pragma unroll
            for (int l = 0; l < ((PROBE & 1) ? 0 : TN); ++l) {
                if (l == 0) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                else __builtin_amdgcn_sched_group_barrier(0x008, Q, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
#pragma unroll
            for (int l = 0; l < ((PROBE & 2) ? 0 : TM); ++l) {
                __builtin_amdgcn_sched_group_barrier(0x008, Q, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);      // whatever MFMAs remain
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    {
        const int a_off = a_chunk_off(0);
#pragma unroll
        for (int u = 0; u < GRP; ++u) {
            const unsigned ab = a_addr0 + (a_off + u * 4 * LI::PSG) * 4;
#pragma unroll
            for (int i = 0; i < TM; ++i) f0.a[u][i] = lds_read4(ab + a_imm(i));
#pragma unroll
            for (int j = 0; j < TN; ++j) f0.b[u][j] = b0[u][j];
        }
    }
    if (PROBE) f1 = f0;
    // (The two waves of a workgroup that share a SIMD do not advance evenly - the older one wins the arbitration and leaves
    // the loop ~12 % earlier.  Alternating s_setprio between them evens that out but the pair's finish time, set by the
    // MFMA pipe, does not move: measured, not kept.)
#pragma unroll 1
    for (int ch = 0; ch + 1 < NCHUNK; ch += 2) {
        stage(f0, f1, ch + 1);
        stage(f1, f0, (ch + 2 < NCHUNK) ? ch + 2 : ch + 1);         // past the end: re-read the last chunk (in bounds, unused)
    }
    if (NCHUNK & 1) {
#pragma unroll
        for (int u = 0; u < GRP; ++u) mfma_group(f0, u);
    }
}

// ---- AFFNET_ARITH_FP32_SPLIT3: the same contraction on split operands (fp32 = three bf16 terms) --------------------------------------
// (round 3's loops on separate term planes, LayB / conv3x3_mfma_s3p: kept for tools/probes/s3_loop_probe.hip, which measures them against
// the round-4 loops the trunks use: LayQ / conv3x3_mfma_s3q below)
// x = x0 + x1 + x2 with every term rounded to bf16 is exact for a 24-bit significand, every bf16 x bf16 product is exact in the fp32
// accumulator of v_mfma_f32_16x16x32_bf16, and the six products with i + j <= 2 carry an fp32 product to 2^-25 relative - at 16x the
// rate of the fp32 MFMA.  Weights are split at pack time: Ws [tap][CIN/32][term][kq][COUT][8 bf16]; activations are split ONCE, by the
// epilogue of the layer that produces them, into three bf16 planes (LayB) - the first version kept them fp32 in LDS and split each
// fragment in registers when it was read (9 taps x NG channel groups times per element): 4.5 VALU instructions per MFMA, matrix pipe
// 49 % busy (round 3, removed).  Accumulator layout = conv3x3_mfma's.  Selected per context (affnet_set_arith).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Exact remainder of a pair after its bf16 roundings u = (bf16(v.x), bf16(v.y)): v_dot2c_f32_bf16 with the constant pair (-1, 0) /
// (0, -1) is  v.x - float(u.lo) + 0 * float(u.hi)  in one instruction; the difference is representable, so the rounding mode does not
// matter.  Checked bit-for-bit against the shift / subtract form on 2^24 random bit patterns incl. denormals - they differ only where
// bf16(v) overflows to inf.  The constants come from s_mov through an asm so that the compiler cannot fold them into an inline
// operand: it encodes the packed bf16 (-1, 0) as the inline constant -1.0, which the hardware does not read as bf16 (the low-half
// remainders came out unchanged).
// Measured alternatives when the split still sat inside the MFMA loops (HardNet conv1, cycles of the slower wave of a SIMD): shift /
// mask + v_pk_add_f32 54.9 k, this form 48.8 k, shift / mask + two unpacked v_sub_f32 50.2 k (pre-split: 38.3 k incl. a second conv0
// pass).  tools/probes/mfma_valu_overlap.hip shows why none of them hides under the matrix pipe: with two waves per SIMD, 12 bf16 MFMAs + 36 VALU instructions take 528-553 cycles for v_fmac / v_cvt_pk /
// v_lshlrev (MFMAs alone 428, the VALU alone 190-330) and ~1000 cycles for v_dot2c / v_pk_add_f32 - VALU work next to bf16 MFMAs is at
// best half hidden, so the remedy is not to have it in the loop (pre-split layouts below).
__device__ __forceinline__ void split_remainder(f32x2& v, unsigned u) {
    unsigned c0, c1;
    asm("s_mov_b32 %0, 0xbf80" : "=s"(c0));
    asm("s_mov_b32 %0, 0xbf800000" : "=s"(c1));
    const bf16x2 b = __builtin_bit_cast(bf16x2, u);
    v.x = __builtin_amdgcn_fdot2_f32_bf16(b, __builtin_bit_cast(bf16x2, c0), v.x, false);
    v.y = __builtin_amdgcn_fdot2_f32_bf16(b, __builtin_bit_cast(bf16x2, c1), v.y, false);
}

// ---- AFFNET_ARITH_FP32_SPLIT2H: fp32 = two fp16 terms, three products ------------------------------------------------------------------
// x ~ h + l, h = fp16(x), l = fp16(x - h) (both round-to-nearest-even; x - h is exact in fp32): 11 + 11 bits + the remainder's sign = 23 of
// fp32's 24 significand bits, |x - h - l| <= 2^-23 |x| for |x| >= 2^-2 and <= 2^-25 ABSOLUTE below (activations are not scaled: the low term is then a subnormal fp16).  w a = w_h a_h + w_l a_h + w_h a_l (+ w_l a_l <= 2^-24, dropped) on v_mfma_f32_16x16x32_f16: every fp16 x fp16 product is exact
// in the fp32 accumulator and subnormal fp16 inputs are honoured (tools/probes/f16_split_probe.hip), so small activations keep an ABSOLUTE
// error of 2^-25.  Half the matrix instructions of the three-term bf16 scheme; the loops and epilogues are the same code with TERMS = 2, on
// a layout of their own (LayR below: 16-byte pixels, two thirds of LayQ's bytes, conflict free for every reader).
// Weights are packed times 2^e per layer (net_layout: w_h2) so that both terms sit in fp16's normal range; the loop multiplies its sums by
// 2^-e (exact).  Activations are not scaled: |a| < 65504 required (include/affnet_hip.h).
// The pair split is written in assembly: this compiler's own lowering of  <2 x float> -> <2 x half>  followed by element reads uses the LOW
// half for both elements (v_cvt_pk_f16_f32, then v_perm / v_cvt_f32_f16 of the low half twice - found by the probe: every odd element wrong).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split_h2_pair(f32x2 v, unsigned& hi, unsigned& lo) {
    float r0, r1;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(v.x), "v"(v.y));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hi), "v"(v.x));                      // x - float(hi.lo16): exact
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hi), "v"(v.y));       // y - float(hi.hi16)
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(lo) : "v"(r0), "v"(r1));
}

// Split four fp32 values (a lane's four consecutive channels) into TERMS terms and store term t at dst + 16 t (8 bytes each: half a cell)
template <int TERMS, int TSTEP = 16>
__device__ __forceinline__ void split_store4(char* dst, f32x4 v) {
    f32x2 lo = {v.x, v.y}, hi = {v.z, v.w};
    if constexpr (TERMS == 2) {
        unsigned h0, l0, h1, l1;
        split_h2_pair(lo, h0, l0);
        split_h2_pair(hi, h1, l1);
        *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(dst + TSTEP) = make_uint2(l0, l1);
    } else {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const unsigned u0 = __builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2));
            const unsigned u1 = __builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2));
            *reinterpret_cast<uint2*>(dst + t * TSTEP) = make_uint2(u0, u1);
            if (t < 2) { split_remainder(lo, u0); split_remainder(hi, u1); }
        }
    }
}

// one matrix instruction of the split arithmetic: fragments travel as 16 bytes, the term count picks the operand type
template <int TERMS>
__device__ __forceinline__ f32x4 split_mfma(bf16x8 w, bf16x8 a, f32x4 c) {
    if constexpr (TERMS == 2) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, a), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, c, 0, 0, 0);
}

// ---- pre-split activations: a layer's output stored as three bf16 planes -------------------------------------------------------
// Splitting in the reading loop is redundant: the NG waves that share a pixel tile (different output channels) each split the same
// fragment - 4.5 VALU instructions per MFMA in the first version (PMC: 8.0e9 VALU vs 1.8e9 MFMA instructions per 32-image HardNet
// launch, VALU and matrix pipe each ~50 % busy, one after the other).  Where the buffer allows (1.5x the fp32 size), the EPILOGUE
// splits every output element once and the next layer reads ready bf16 fragments: element (term t, channel c, y, x) of an H x H layer
// sits at  t * TS + (c / 8) * GS + ((y + 1) * WP + x + 1) * 16 + (c % 8) * 2  bytes - one ds_read_b128 = the 8 channels of one term
// of one pixel = a lane's B fragment of a k = 32 step.
// Bank conflicts (ds_read_b128 is served in four groups of 16 lanes - {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... - over a 256-byte
// bank window): pixels {0-3, 12-15} of lane quarter kq and pixels {4-11} of quarter kq + 1 share a group, so the 8-channel group stride GS
// decides whether their 16-byte cells collide.  The first version had GS = 64 (mod 256) everywhere: 56 % of the LDS-array cycles of the
// split HardNet launch were conflict cycles (SQ_LDS_BANK_CONFLICT 2.9e9 of SQ_LDS_IDX_ACTIVE 5.1e9).  GS is rounded up to a multiple of
// 256 plus GREM, chosen per READER:  16 pixels contiguous (stride-1 reader of a 16 / 32-wide layer): GREM = 0;  2 rows x 8 pixels (8-wide
// layer, row stride 256 bytes = WP 16): GREM = 128;  16 pixels at a 32-byte pitch (stride-2 reader of a 32-wide layer): GREM = 16.
template <int H_, int W_, int WP_, int C_, int GREM_ = 0>
struct LayB {
    static constexpr int H = H_, W = W_, WP = WP_, C = C_;      // H rows x W columns (+ a one-cell halo), row stride WP cells
    static constexpr int GS = (((H_ + 2) * WP_ * 16 + 255) / 256) * 256 + GREM_;      // bytes per 8-channel group
    static constexpr int TS = (C_ / 8) * GS;              // bytes per term
    static constexpr int BYTES = 3 * TS;
};

// The contraction on a PRE-SPLIT input (layout LI = LayB): no VALU in the loop - three ds_read_b128 per pixel tile and k = 32 step.
template <int NW, int CIN, int COUT, typename LI, int STRIDE, int TM, int TN>
__device__ __forceinline__ void conv3x3_mfma_s3p(const float* act, const float* __restrict__ Ws, f32x4 (&acc)[TM][TN], int wave, int lane, bool alt_prio) {
    constexpr int HOUT = LI::H / STRIDE, WOUT = LI::W / STRIDE;
    constexpr int MT = HOUT * WOUT / 16, NT = COUT / 16;
    constexpr int MG = MT / TM, NG = NT / TN;
    constexpr int NG32 = CIN / 32, NS = 9 * NG32;
    static_assert(MG * NG == NW && CIN % 32 == 0 && LI::C == CIN, "bad tiling for the split-operand loop");
    const int mg = wave % MG, ng = wave / MG;
    const int m = lane & 15, kq = lane >> 4;
    int a_lane;                                                            // bytes
    {
        const int p = mg * TM * 16 + m;
        const int oy = p / WOUT, ox = p - oy * WOUT;
        a_lane = kq * LI::GS + ((oy * STRIDE) * LI::WP + ox * STRIDE) * 16;
    }
    const unsigned a_addr0 = lds_byte_addr(act) + a_lane;
    auto a_imm = [](int i) { return 16 * (WOUT == 8 ? i * 2 * STRIDE * LI::WP : (((i * 16) / WOUT) * STRIDE * LI::WP + ((i * 16) % WOUT) * STRIDE)); };
    constexpr int WS_FLOATS = 9 * (CIN / 32) * 3 * 4 * COUT * 4;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Ws, WS_FLOATS);
    const int w_lane = (kq * COUT + ng * TN * 16 + m) * 16;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 w[2][3][TN];
    auto load_w = [&](bf16x8 (&dst)[3][TN], int s) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                dst[t][j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, w_lane + j * 256, ((s * 3 + t) * 4 * COUT) * 16, 0));
    };
    // Rotating schedule: the fragments of pixel tile i for step s + 1 are requested right after tile i's MFMAs of step s were issued
    // (same registers - the matrix pipe has read them by then), so every ds_read has the other tiles' MFMAs (>= 100 issue cycles) to
    // complete.  The first version read a step's 3 TM fragments at its top and waited: a wave stalled once per step and the two waves
    // of a SIMD drifted apart (conv3: faster wave 30 k cycles, slower 35 k; matrix-pipe floor 27.6 k).
    auto frag_addr = [&](int s) {
        const int tap = s / NG32, G = s - tap * NG32;
        const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;
        return a_addr0 + 4 * G * LI::GS + (ky * LI::WP + kx) * 16;
    };
    bf16x8 a[TM][3];
    auto read_tile = [&](unsigned ab, int i) {
#pragma unroll
        for (int t = 0; t < 3; ++t) a[i][t] = __builtin_bit_cast(bf16x8, lds_read4(ab + a_imm(i) + t * LI::TS));
    };
    auto step = [&](const bf16x8 (&wc)[3][TN], int s_next) {
        if (alt_prio) {                       // the two waves of a SIMD (w, w + 4) take turns at the higher priority, one step each
            if ((s_next ^ (wave >> 2)) & 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        const unsigned ab = frag_addr(s_next);
        constexpr int TW[6] = {0, 1, 2, 0, 1, 0}, TA[6] = {2, 1, 0, 1, 0, 0};      // smallest terms first
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wc[TW[t]][j], a[i][TA[t]], acc[i][j], 0, 0, 0);
            read_tile(ab, i);
            __builtin_amdgcn_sched_group_barrier(0x008, 6 * TN, 0);      // this tile's MFMAs ...
            __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);           // ... then its three reads for the next step
        }
    };
    load_w(w[0], 0);
#pragma unroll
    for (int i = 0; i < TM; ++i) read_tile(frag_addr(0), i);
#pragma unroll 1
    for (int s = 0; s + 1 < NS; s += 2) {
        load_w(w[1], s + 1);
        step(w[0], s + 1);
        load_w(w[0], (s + 2 < NS) ? s + 2 : s + 1);
        step(w[1], (s + 2 < NS) ? s + 2 : s + 1);                        // the last step re-reads its own fragments (never used)
    }
    if (NS & 1) step(w[0], NS - 1);
    if (alt_prio) __builtin_amdgcn_s_setprio(0);
}

// ---- round 4: term-interleaved pre-split layout + term-major MFMA order ------------------------------------------------------------
// LayB keeps the three bf16 planes of a layer TS bytes apart.  2 * TS exceeds the 16-bit DS offset field for every layer here, so each
// fragment read of the loops above needed its own v_add_u32 (3 per pixel tile and step) and the hazard s_nops the compiler puts between an
// MFMA and a VALU write of a register the MFMA reads - inside the MFMA stream.  LayQ interleaves the terms INSIDE the pixel cell:
// element (term t, channel c, y, x) sits at  (c / 8) * GS + ((y + 1) * WP + x + 1) * 48 + t * 16 + (c % 8) * 2  bytes, so the three
// terms of a lane's fragment are one address + immediates 0 / 16 / 32, the tiles of a wave further immediates, and a k = 32 step costs ONE
// v_add (step offset, an SGPR) instead of 3 TM.  Bank behaviour of the 48-byte pixel pitch (ds_read_b128, 16-lane service groups, tools/
// bank model in DESIGN.md): 16 pixels of a row at 48 B cover the 64 banks exactly once (12 m mod 64 are the sixteen multiples of 4), so
// the stride-1 readers are conflict free with GS = 0 (mod 256); 16 pixels at a 96 B pitch (stride-2 reader of a 32-wide layer) with
// GS = 16 (mod 256); two rows of 8 pixels with a 768 B row pitch (8-wide layers, WP = 16) with GS = 128 (mod 256).  Only the stride-2
// reader of the 16-wide layers (conv4) keeps 2-way conflicts: its row pitch 2 * 18 * 48 B would have to be a multiple of 256 B (WP = 24:
// 166 KB for the 64-channel layers).
template <int H_, int W_, int WP_, int C_, int GREM_ = 0, int TERMS_ = 3>
struct LayQ {
    static constexpr int H = H_, W = W_, WP = WP_, C = C_;      // H rows x W columns (+ a one-cell halo), row stride WP cells of 48 bytes
    static constexpr int GREM = GREM_;
    static constexpr int TERMS = TERMS_;                        // 3 bf16 terms or 2 fp16 terms per element (the cell keeps three 16-byte slots either way)
    static constexpr int CELL = 48;
    // address pitches (bytes) every user goes through: right neighbour, the pixel below, next term of the same pixel; 16-byte slots per pixel
    static constexpr int PIXB = CELL, ROWB = WP_ * CELL, TSTEP = 16, SLOTS = 3;
    __device__ __host__ static constexpr int at(int y, int x) { return y * ROWB + x * PIXB; }      // (y, x) counted from the top-left halo cell
    static constexpr int GS = (((H_ + 2) * ROWB + 255) / 256) * 256 + GREM_;      // bytes per 8-channel group
    static constexpr int BYTES = (C_ / 8) * GS;
};

// Two-term layout with a 16-byte pixel pitch (AFFNET_ARITH_FP32_SPLIT2H): the hi cells and the lo cells of a ROW sit side by side - element (term t, channel c, y, x) at
//   (c / 8) * GS + (y + 1) * ROWB + t * (WP * 16) + (x + 1) * 16 + (c % 8) * 2,   ROWB = 2 * WP * 16 bytes
// - two thirds of LayQ's bytes (HardNet's conv0 output of a WHOLE patch fits: 148 KB), the second term still one immediate away, and with the pixel pitch a
// divisor of the 256-byte bank window every reader of the trunks can be made conflict free (ds_read_b128 service groups {0-3, 12-15, 20-27} ..., 16-byte slots
// mod 16; kq = lane quarter, its 8-channel group GS bytes further):
//   stride 1, one-row tiles (32- / 16-wide layers): pixels 0-3, 12-15 of quarter kq and 4-11 of kq + 1 fill the 16 slots once with GS = 0 (mod 256);
//   stride 1, two rows x 8 pixels (8-wide layers): the second row must start 8 slots later: ROWB / 16 = 2 WP = 8 (mod 16): WP = 12, GS = 0 (mod 256);
//   stride 2, one-row tiles (32-wide input): pixel pitch 32 B = even slots only; quarter kq + 1 takes the odd ones with GS = 16 (mod 256);
//   stride 2, two rows x 8 (16-wide input): rows 2 apart must start on the same slot: 4 WP = 0 (mod 16): WP = 20, and GS = 16 (mod 256) - the reader that
//   kept 2-way conflicts in LayQ (conv4).
// HALLOC_ = rows the group stride is sized for (default H + 2): a 16-row VIEW of a 32-row layout (the half-patch loops of conv1 / conv2) has HALLOC_ = 34
template <int H_, int W_, int WP_, int C_, int GREM_ = 0, int HALLOC_ = H_ + 2>
struct LayR {
    static constexpr int H = H_, W = W_, WP = WP_, C = C_, GREM = GREM_;
    static constexpr int TERMS = 2, SLOTS = 2;
    static constexpr int PIXB = 16, ROWB = 2 * WP_ * 16, TSTEP = WP_ * 16;
    __device__ __host__ static constexpr int at(int y, int x) { return y * ROWB + x * PIXB; }
    static constexpr int GS = ((HALLOC_ * ROWB + 255) / 256) * 256 + GREM_;
    static constexpr int BYTES = (C_ / 8) * GS;
};

template <typename L, int NTHR>
__device__ __forceinline__ void zero_halo_q(float* act, int tid = threadIdx.x) {
    constexpr int H = L::H, W = L::W, CELLS = 2 * (W + 2) + 2 * H, GROUPS = L::C / 8;
    char* base = reinterpret_cast<char*>(act);
    for (int i = tid; i < GROUPS * CELLS * L::SLOTS; i += NTHR) {    // one 16-byte store = one term of one halo cell
        const int t = i % L::SLOTS, ce = i / L::SLOTS;
        const int g = ce / CELLS, e = ce - g * CELLS;
        int y, x;
        if (e < W + 2) { y = 0; x = e; }
        else if (e < 2 * (W + 2)) { y = H + 1; x = e - (W + 2); }
        else { const int r = e - 2 * (W + 2); y = 1 + (r >> 1); x = (r & 1) ? W + 1 : 0; }
        *reinterpret_cast<f32x4*>(base + (size_t)g * L::GS + L::at(y, x) + t * L::TSTEP) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
}

// The epilogues' ReLU and + bias, ReLU of one float4 (the lane's four channels of a pixel)
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    v.x = fmaxf(v.x, 0.0f); v.y = fmaxf(v.y, 0.0f); v.z = fmaxf(v.z, 0.0f); v.w = fmaxf(v.w, 0.0f);
    return v;
}
__device__ __forceinline__ f32x4 bias_relu(f32x4 y, f32x4 bias) { return relu4(y + bias); }

// (+ bias,) ReLU, split into three bf16 terms, store ONE pixel tile into a LayQ layout: `cell` = byte offset of the lane's pixel cell
template <typename LO, int TN, bool ADD_BIAS = true>
__device__ __forceinline__ void split_store_tile_q(char* base, int cell, int nt0, const f32x4 (&bias)[TN], const f32x4 (&acc)[TN], int g) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const f32x4 v = ADD_BIAS ? bias_relu(acc[j], bias[j]) : relu4(acc[j]);
        const int c0 = (nt0 + j) * 16 + 4 * g;                           // first of this lane's 4 channels
        char* dst = base + (c0 >> 3) * LO::GS + cell + (c0 & 4) * 2;
        split_store4<LO::TERMS, LO::TSTEP>(dst, v);
    }
}

template <int COUT, typename LO, int TM, int TN, int HT = LO::H>
__device__ __forceinline__ void store_tiles_split_q(float* act, const f32x4 (&bias)[TN], const f32x4 (&acc)[TM][TN], int wave, int lane, int row_off = 0) {
    constexpr int W = LO::W;
    constexpr int MT = HT * W / 16, MG = MT / TM;
    const int mg = wave % MG, ng = wave / MG;
    const int n = lane & 15, g = lane >> 4;
    char* base = reinterpret_cast<char*>(act);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int p = (mg * TM + i) * 16 + n;
        const int oy = p / W, ox = p - oy * W;
        split_store_tile_q<LO, TN>(base, LO::at(oy + row_off + 1, ox + 1), ng * TN, bias, acc[i], g);
    }
}

template <int N> struct IntC { static constexpr int v = N; };

// Weight fragments of one k = 32 step of a split layer: [term][channel tile] (two-term arithmetic leaves w[2] unused: no registers)
template <int TN>
struct S3W {
    bf16x8 w[3][TN];
};

// Lane part of the weight address of a split layer (bytes): the step offset is an SGPR, the tile offset an immediate
template <int NW, int COUT, int MG, int TN>
__device__ __forceinline__ int s3_w_lane(int wave, int lane) {
    return (((lane >> 4) * COUT) + (wave / MG) * TN * 16 + (lane & 15)) * 16;
}
template <int COUT, int TN, int TERMS = 3>
__device__ __forceinline__ void s3_load_w(S3W<TN>& dst, __amdgpu_buffer_rsrc_t wrsrc, int w_lane, int s) {
#pragma unroll
    for (int t = 0; t < TERMS; ++t)
#pragma unroll
        for (int j = 0; j < TN; ++j)
            dst.w[t][j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, w_lane + j * 256, ((s * TERMS + t) * 4 * COUT) * 16, 0));
}
// The first step's weights of a layer do not depend on the activations: requested BEFORE the barriers / epilogue of the previous layer
// (1 - 2 k cycles of L2 latency under load, otherwise paid with an idle matrix pipe at the head of every loop).
template <int NW, int CIN, int COUT, int HOUT_TILES, int TM, int TN, int TERMS = 3>
__device__ __forceinline__ void s3_prefetch_w0(const float* __restrict__ Ws, S3W<TN>& w0, int wave, int lane) {
    constexpr int MG = HOUT_TILES / TM;
    constexpr int WS_FLOATS = (CIN == 16 ? 5 : 9 * (CIN / 32)) * TERMS * 4 * COUT * 4;
    s3_load_w<COUT, TN, TERMS>(w0, weight_rsrc(Ws, WS_FLOATS), s3_w_lane<NW, COUT, MG, TN>(wave, lane), 0);
}

// The contraction on a term-interleaved pre-split input (LI = LayQ).  MFMA order is TERM-MAJOR: a term pair (w_i, a_j) runs over all
// TM x TN tiles of the wave before the next pair starts, so consecutive MFMAs never share an accumulator (the tile-major order of
// conv3x3_mfma_s3p chained six dependent MFMAs per accumulator, two chains interleaved) and the activation terms retire one after the
// other: pairs (w0 a0, w1 a0, w2 a0) - a0 dead, its registers take the NEXT step's a0 - (w0 a1, w1 a1) - a1 reloaded - (w0 a2) - a2
// reloaded.  Every fragment read has >= 24 MFMAs (a0), 32 (a1), 40 (a2) of this wave between issue and use.  The order of the six pairs
// inside a step does not matter numerically: the fp32 accumulator already carries the sum over all previous steps.
// C16 = true: 16 input channels (AffNet / OriNet conv1, conv2): one k = 32 step = two taps x 16 channels (lane quarter kq: tap 2 s + (kq >> 1),
// channel group kq & 1), 5 steps, the pad half-step re-reads tap 8 against zero weights.
// PROBE (tools/probes/s3_loop_probe.hip only): bit 0 = no weight loads inside the loop, bit 1 = no fragment reloads, bits 4.. = s_nop pacing
template <int NW, int CIN, int COUT, typename LI, int STRIDE, int TM, int TN, int PROBE = 0>
__device__ __forceinline__ void conv3x3_mfma_s3q(const float* act, const float* __restrict__ Ws, const S3W<TN>& w_first, f32x4 (&acc)[TM][TN],
                                                 int wave, int lane, int variant) {
    const bool alt_prio = (variant & 1) != 0;      // affnet_debug_split3_variant bits: 0 = alternating wave priorities, 1 = (A/B only) skip the NaN -> inf step of the two-term loops
    constexpr bool C16 = (CIN == 16);
    constexpr int TERMS = LI::TERMS;                                       // 3: bf16 terms, six products; 2: fp16 terms, three products (w_h a_h, w_l a_h, w_h a_l)
    constexpr int HOUT = LI::H / STRIDE, WOUT = LI::W / STRIDE;
    constexpr int MT = HOUT * WOUT / 16, NT = COUT / 16;
    constexpr int MG = MT / TM, NG = NT / TN;
    constexpr int NG32 = C16 ? 1 : CIN / 32, NS = C16 ? 5 : 9 * NG32;
    static_assert(MG * NG == NW && (C16 || CIN % 32 == 0) && LI::C == CIN && (TERMS == 2 || TERMS == 3), "bad tiling for the split-operand loop");
    const int mg = wave % MG;
    const int m = lane & 15, kq = lane >> 4;
    int a_lane;                                                            // bytes
    {
        const int p = mg * TM * 16 + m;
        const int oy = p / WOUT, ox = p - oy * WOUT;
        a_lane = (C16 ? (kq & 1) : kq) * LI::GS + LI::at(oy * STRIDE, ox * STRIDE);
    }
    const unsigned a_addr0 = lds_byte_addr(act) + a_lane;
    auto a_imm = [](int i) { return WOUT == 8 ? LI::at(i * 2 * STRIDE, 0) : LI::at(((i * 16) / WOUT) * STRIDE, ((i * 16) % WOUT) * STRIDE); };
    static_assert(LI::at(TM * 2 * STRIDE, 0) + 2 * LI::TSTEP < 65536, "tile immediates must fit the DS offset field");
    constexpr int WS_FLOATS = (C16 ? 5 : 9 * NG32) * TERMS * 4 * COUT * 4;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Ws, WS_FLOATS);
    const int w_lane = s3_w_lane<NW, COUT, MG, TN>(wave, lane);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto frag_addr = [&](int s) -> unsigned {
        if (C16) {
            const int ta = 2 * s, tb = (2 * s + 1 < 9) ? 2 * s + 1 : 8;
            const int off_a = LI::at(ta / 3, ta % 3), off_b = LI::at(tb / 3, tb % 3);
            return a_addr0 + ((kq >> 1) ? off_b : off_a);
        }
        const int tap = s / NG32, G = s - tap * NG32;
        const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;
        return a_addr0 + 4 * G * LI::GS + LI::at(ky, kx);
    };
    bf16x8 a[TM][TERMS];
    S3W<TN> wb[2];
    wb[0] = w_first;
    {
        const unsigned ab = frag_addr(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int t = 0; t < TERMS; ++t) a[i][t] = __builtin_bit_cast(bf16x8, lds_read4(ab + a_imm(i) + t * LI::TSTEP));
    }
    auto pair_mfma = [&](const S3W<TN>& wc, int tw, int ta) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = split_mfma<TERMS>(wc.w[tw][j], a[i][ta], acc[i][j]);
                if constexpr ((PROBE >> 4) != 0) __builtin_amdgcn_sched_barrier(0);
                if constexpr ((PROBE >> 4) != 0) asm volatile("s_nop %0" ::"n"((PROBE >> 4) - 1));
                if constexpr ((PROBE >> 4) != 0) __builtin_amdgcn_sched_barrier(0);
            }
    };
    auto reload = [&](unsigned ab, int t) {
        if constexpr (PROBE & 2) return;
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i][t] = __builtin_bit_cast(bf16x8, lds_read4(ab + a_imm(i) + t * LI::TSTEP));
    };
    constexpr int NT_ = TM * TN;
    // the term pairs of one step in term-major order, every activation term reloaded (for the next step) right after its last use;
    // then the pinned interleaving: NLEAD weight loads, one after each of the first MFMAs, and the fragment reads where their registers die
    auto pairs = [&](const S3W<TN>& wc, unsigned ab, bool load_next) {
        if constexpr (TERMS == 3) {
            pair_mfma(wc, 0, 0); pair_mfma(wc, 1, 0); pair_mfma(wc, 2, 0);
            if (load_next) reload(ab, 0);
            pair_mfma(wc, 0, 1); pair_mfma(wc, 1, 1);
            if (load_next) reload(ab, 1);
            pair_mfma(wc, 0, 2);
            if (load_next) reload(ab, 2);
        } else {
            pair_mfma(wc, 0, 0); pair_mfma(wc, 1, 0);
            if (load_next) reload(ab, 0);
            pair_mfma(wc, 0, 1);
            if (load_next) reload(ab, 1);
        }
    };
    auto pin = [&](auto n_lead_c) {
        constexpr int n_lead = decltype(n_lead_c)::v;
#pragma unroll
        for (int l = 0; l < n_lead; ++l) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, TERMS * NT_ - n_lead, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, TM, 0);
        if constexpr (TERMS == 3) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * NT_, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, TM, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NT_, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, TM, 0);
    };
    // one step: weights of step s_next requested first (spread between the first MFMAs), fragments of s_next as the terms retire
    const int wave_hi = __builtin_amdgcn_readfirstlane(wave >> 2);      // scalar: the priority switch below must not become a divergent branch
    // (Tried in round 4, profiles/r04_s3_s3_loop_probe_fair_priorities.txt: "fair" priorities - the two waves of a SIMD publish the step they are in
    // through LDS and the one that is AHEAD lowers its issue priority, so that the pair advances together instead of the older wave taking ~3/4 of the
    // pipe and the younger one finishing alone.  Slower on every shape (conv3 87.9 % of the pipe floor vs 91.5 %, conv5 77.8 vs 87.0): the arbiter's
    // oldest-first order wastes less than two waves that stall on the same things at the same time.  Removed.)
    auto step = [&](const S3W<TN>& wc, S3W<TN>& wn, int s_next, bool load_next) {
        if (alt_prio) {                       // the two waves of a SIMD (w, w + 4) take turns at the higher priority, one step each
            if ((s_next ^ wave_hi) & 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        unsigned ab = frag_addr(s_next);
        asm("" : "+v"(ab));
        if constexpr (PROBE & 1) { if (load_next) wn = wc; }
        else { if (load_next) s3_load_w<COUT, TN, TERMS>(wn, wrsrc, w_lane, s_next); }
        pairs(wc, ab, load_next);
        if (load_next && PROBE == 0) pin(IntC<TERMS * TN>{});
        __builtin_amdgcn_sched_barrier(0);
    };
    static_assert(TERMS * TN <= TERMS * TM * TN, "weight loads are spread over the first term pairs");
    auto finish = [&]() {
        if constexpr (TERMS == 2) {           // the two-term weights are packed times 2^e (fp16 range): undo it, exactly
            const float osc = Ws[WS_FLOATS];
            // An activation beyond fp16's range (|a| >= 65520) splits into (inf, -inf) and its products sum to NaN - which the ReLU of every epilogue
            // (v_max_f32 returns the non-NaN operand) would turn into a plausible 0.  NaN -> +inf here: +inf survives bias + ReLU, splits into (inf, NaN)
            // in the next layer and arrives at the outputs as inf / NaN (HardNet: NaN descriptors) instead of passing silently.
            if (variant & 2) {                                             // (A/B of this step's cost: tools/ab_nan_step.py)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] *= osc;
                return;
            }
            f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) { acc[i][j] *= osc; sum += acc[i][j]; }
            const float s1 = (sum.x + sum.y) + (sum.z + sum.w);            // NaN iff a NaN (or +inf and -inf) is among the wave's sums: rare path below
            if (__builtin_amdgcn_ballot_w64(s1 != s1) != 0) {
                const float pinf = __builtin_inff();
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        f32x4 v = acc[i][j];
                        v.x = (v.x == v.x) ? v.x : pinf; v.y = (v.y == v.y) ? v.y : pinf; v.z = (v.z == v.z) ? v.z : pinf; v.w = (v.w == v.w) ? v.w : pinf;
                        acc[i][j] = v;
                    }
            }
        }
    };
    if constexpr (C16) {
        // 16 input channels (5 steps, fully unrolled; AffNet / OriNet conv1, conv2 at 128 VGPRs and four waves per SIMD): ONE weight set,
        // the next step's fragments are requested when the current step's last term pair has been issued - the other waves of the SIMD
        // cover the L2 round trip (a second set cost 8 - 10 spilled registers here)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bool more = s + 1 < NS;
            unsigned ab = frag_addr(more ? s + 1 : s);
            asm("" : "+v"(ab));
            pairs(wb[0], ab, more);
            if (more) {
                pin(IntC<0>{});
                __builtin_amdgcn_sched_barrier(0);
                s3_load_w<COUT, TN, TERMS>(wb[0], wrsrc, w_lane, s + 1);
            }
        }
        finish();
        return;
    }
    // (Tried for the two-term loops, whose steps have half the matrix time to cover the L2 round trip of the weight fragments: weights requested TWO steps
    // ahead through three rotating sets.  profiles/r04_s4_s3_loop_probe_split2h_prefetch_depth.txt: -4 .. +2.5 % per layer shape, HardNet trunk 9.08 vs 9.13 ms
    // per 48000 patches at 255 instead of 190 VGPRs - the weights are not what these loops wait for.  Removed.)
#pragma unroll 1
    for (int s = 0; s + 2 < NS; s += 2) {
        step(wb[0], wb[1], s + 1, true);
        step(wb[1], wb[0], s + 2, true);
    }
    if (NS & 1) {                             // NS odd: the loop left the last step in wb[0]
        step(wb[0], wb[1], NS - 1, false);
    } else {
        step(wb[0], wb[1], NS - 1, true);
        step(wb[1], wb[0], NS - 1, false);
    }
    if (alt_prio) __builtin_amdgcn_s_setprio(0);
    finish();
}

// The same into a term-interleaved layout (LayQ).
template <int NW, typename LQH, int TN>
__device__ __forceinline__ void conv0_half_split_q(const float* patch, const float (&b)[3][TN], const f32x4 (&bv)[TN], float* act, int pass,
                                                   int wave, int lane) {
    static_assert(NW == 8 && LQH::H == 16 && LQH::W == 32 && LQH::C == 16 * TN, "half-patch conv0: 8 waves, all channel tiles in every wave");
    const int m = lane & 15, kq = lane >> 4;
    int toff[3];
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3) {
        const int t = 4 * s3 + kq;
        toff[s3] = t < 9 ? (t / 3) * WP32 + (t % 3) : 0;
    }
    char* base = reinterpret_cast<char*>(act);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        int row_l, x0;
        if (k < 4) { const int T = 4 * wave + k; row_l = T >> 1; x0 = (T & 1) * 16; }
        else { row_l = pass ? -1 : 16; x0 = (wave & 1) * 16; }
        const int pb = (row_l + 16 * pass) * WP32 + x0 + m;
        float av[3];
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3) av[s3] = patch[pb + toff[s3]];
        f32x4 acc[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = bv[j];
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[s3][j], av[s3], acc[j], 0, 0, 0);
        split_store_tile_q<LQH, TN, false>(base, LQH::at(row_l + 1, x0 + m + 1), 0, bv, acc, kq);
    }
}

// conv0 of a WHOLE 32 x 32 patch straight into a pre-split layout L (32 rows x 32 columns; two-term arithmetic: LayR holds it in 145 KB for 32 channels)
template <int NW, typename L, int TN>
__device__ __forceinline__ void conv0_whole_split_q(const float* patch, const float (&b)[3][TN], const f32x4 (&bv)[TN], float* act, int wave, int lane) {
    static_assert(NW == 8 && L::H == 32 && L::W == 32 && L::C == 16 * TN, "whole-patch conv0: 8 waves x 8 pixel tiles, all channel tiles in every wave");
    const int m = lane & 15, kq = lane >> 4;
    int toff[3];
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3) {
        const int t = 4 * s3 + kq;
        toff[s3] = t < 9 ? (t / 3) * WP32 + (t % 3) : 0;
    }
    char* base = reinterpret_cast<char*>(act);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int T = 8 * wave + k, row = T >> 1, x0 = (T & 1) * 16;
        const int pb = row * WP32 + x0 + m;
        float av[3];
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3) av[s3] = patch[pb + toff[s3]];
        f32x4 acc[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = bv[j];
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[s3][j], av[s3], acc[j], 0, 0, 0);
        split_store_tile_q<L, TN, false>(base, L::at(row + 1, x0 + m + 1), 0, bv, acc, kq);
    }
}

// Same contraction with ONE A register set that is reloaded in place (for TM = 8 under a 128-VGPR budget, where two
// sets of 8 float4 do not fit): chunk = one plane group; the tiles are processed in pairs - 8 * TN MFMAs on 2 * TN
// independent accumulators - and as soon as a pair's MFMAs have issued, its two A registers are reloaded with the next
// chunk's data, so every load is (TM - 2) / TM of a chunk ahead of its use.  B fragments keep two sets.
template <int NW, int CIN, int COUT, typename LI, int STRIDE, int TM, int TN>
__device__ __forceinline__ void conv3x3_mfma_roll(const float* act, const float* __restrict__ Wg, const f32x4 (&b0)[1][TN],
                                                  f32x4 (&acc)[TM][TN], int wave, int lane) {
    constexpr int HOUT = LI::H / STRIDE;
    constexpr int MT = HOUT * HOUT / 16, NT = COUT / 16;
    constexpr int MG = MT / TM, NG = NT / TN;
    constexpr int NGRP = CIN / 16, NCHUNK = 9 * NGRP;
    static_assert(MG * NG == NW && TM % 2 == 0 && CIN % 16 == 0, "bad tiling");
    const int mg = wave % MG, ng = wave / MG;
    const int m = lane & 15, kq = lane >> 4;
    // lane address of tile 0 / N-tile 0; the other tiles of the wave sit at compile-time offsets (immediates)
    static_assert(HOUT == 8 || (TM * 16) % HOUT == 0 || HOUT % (TM * 16) == 0, "tile offsets must be wave-uniform constants");
    int a_lane;
    {
        const int p = mg * TM * 16 + m;
        const int oy = p / HOUT, ox = p - oy * HOUT;
        a_lane = kq * LI::PSG + ((oy * STRIDE) * LI::WP + ox * STRIDE) * 4;
    }
    const int b_lane = (kq * COUT + ng * TN * 16 + m) * 4;
    const unsigned a_addr0 = lds_byte_addr(act) + a_lane * 4;
    auto a_imm = [](int i) {                               // byte offset of tile i from tile 0 (compile-time after unrolling)
        return 4 * (HOUT == 8 ? i * 2 * STRIDE * LI::WP * 4 : (((i * 16) / HOUT) * STRIDE * LI::WP + ((i * 16) % HOUT) * STRIDE) * 4);
    };
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wg, 9 * CIN * COUT);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto a_chunk_off = [](int ch) {
        const int tap = ch / NGRP, g0 = ch - tap * NGRP;
        const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;
        return g0 * 4 * LI::PSG + (ky * LI::WP + kx) * 4;
    };
    f32x4 fa[TM], fb0[TN], fb1[TN];
    {
        const int a_off = a_chunk_off(0);
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = lds_read4(a_addr0 + a_off * 4 + a_imm(i));
#pragma unroll
        for (int j = 0; j < TN; ++j) fb0[j] = b0[0][j];
    }
    auto chunk = [&](const f32x4 (&bc)[TN], f32x4 (&bn)[TN], int nxt_ch) {
        unsigned ab = a_addr0 + a_chunk_off(nxt_ch) * 4;
        asm("" : "+v"(ab));
#pragma unroll
        for (int j = 0; j < TN; ++j) bn[j] = buf_read4(wrsrc, b_lane * 4 + j * 256, nxt_ch * (16 * COUT) * 4);
#pragma unroll
        for (int ip = 0; ip < TM; ip += 2) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int i = ip; i < ip + 2; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bc[j][s4], fa[i][s4], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = ip; i < ip + 2; ++i) fa[i] = lds_read4(ab + a_imm(i));
        }
    };
#pragma unroll 1
    for (int ch = 0; ch + 1 < NCHUNK; ch += 2) {
        chunk(fb0, fb1, ch + 1);
        chunk(fb1, fb0, (ch + 2 < NCHUNK) ? ch + 2 : ch + 1);
    }
    if (NCHUNK & 1) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb0[j][s4], fa[i][s4], acc[i][j], 0, 0, 0);
    }
}

// conv0 (1 -> COUT channels, K = 9 taps padded to 12) on the matrix cores as well: A[m][k] = the padded standardised
// patch at (pixel m, tap k), B = packed [12][COUT] taps (rows 9..11 zero), accumulators start at the bias, so the result
// is the fmaf chain bias, tap 0, ..., tap 8 (+ three exact fma(x, 0, acc)).  3 MFMAs per tile instead of 9 * COUT VALU
// FMAs per pixel behind dependent LDS weight reads.
template <int NW, int COUT, int TM, int TN>
__device__ __forceinline__ void conv0_load_w(const float* __restrict__ W0, const float* __restrict__ bias, float (&b)[3][TN],
                                             f32x4 (&bv)[TN], int wave, int lane) {
    constexpr int MG = 64 / TM;
    const int ng = wave / MG, m = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = (ng * TN + j) * 16 + m;
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3) b[s3][j] = W0[(4 * s3 + kq) * COUT + n];
        bv[j] = *reinterpret_cast<const f32x4*>(&bias[(ng * TN + j) * 16 + 4 * kq]);     // accumulator rows 4g..4g+3 = channels
    }
}

template <int NW, int COUT, int TM, int TN>
__device__ __forceinline__ void conv0_mfma(const float* patch, const float (&b)[3][TN], const f32x4 (&bv)[TN], f32x4 (&acc)[TM][TN],
                                           int wave, int lane) {
    constexpr int MT = 64, NT = COUT / 16, MG = MT / TM, NG = NT / TN;
    static_assert(MG * NG == NW, "the waves must tile the layer exactly");
    const int mg = wave % MG;
    const int m = lane & 15, kq = lane >> 4;
    int toff[3];
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3) {
        const int t = 4 * s3 + kq;
        toff[s3] = t < 9 ? (t / 3) * WP32 + (t % 3) : 0;            // taps 9..11: any valid address (weight is zero)
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[i][j] = bv[j];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int p = (mg * TM + i) * 16 + m;
        const int base = (p >> 5) * WP32 + (p & 31);
        float av[3];
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3) av[s3] = patch[base + toff[s3]];
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[s3][j], av[s3], acc[i][j], 0, 0, 0);
    }
}

// Epilogue: (+ bias,) ReLU, write the wave's tiles into the LDS layout LO read by the NEXT layer: lane (n = pixel of the
// tile, g) holds channels 4g..4g+3 -> one float4 of plane group (N-tile * 4 + g).
template <int COUT, typename LO, int TM, int TN, bool ADD_BIAS = true>
__device__ __forceinline__ void store_tiles_lds(float* act, const f32x4 (&bias)[TN], const f32x4 (&acc)[TM][TN], int wave, int lane) {
    constexpr int HOUT = LO::H;
    constexpr int MT = HOUT * HOUT / 16, MG = MT / TM;
    const int mg = wave % MG, ng = wave / MG;
    const int n = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int p = (mg * TM + i) * 16 + n;
        const int oy = p / HOUT, ox = p - oy * HOUT;
        const int pbase = ((oy + 1) * LO::WP + ox + 1) * 4;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const f32x4 v = ADD_BIAS ? bias_relu(acc[i][j], bias[j]) : relu4(acc[i][j]);
            *reinterpret_cast<f32x4*>(&act[((ng * TN + j) * 4 + g) * LO::PSG + pbase]) = v;
        }
    }
}

// Same for the last trunk layer of HardNet: global [pixel p][channel c] = the head GEMM's K order (float4 = 4 channels).
template <int COUT, int TM, int TN>
__device__ __forceinline__ void store_tiles_global(float* __restrict__ dst, const f32x4 (&bias)[TN], const f32x4 (&acc)[TM][TN],
                                                   int wave, int lane) {
    constexpr int MT = 4, MG = MT / TM;
    const int mg = wave % MG, ng = wave / MG;
    const int n = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int p = (mg * TM + i) * 16 + n;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const f32x4 v = bias_relu(acc[i][j], bias[j]);
            *reinterpret_cast<f32x4*>(dst + p * COUT + (ng * TN + j) * 16 + 4 * g) = v;
        }
    }
}


// ---- Winograd F(2x2, 3x3) on v_mfma_f32_16x16x4_f32 (the stride-1 layers of the exact HardNet and OriNet trunks) -------------------
// A 2x2 output tile is  Y = A^T [ (G g G^T) (.) (B^T d B) ] A  over its 4x4 input window d: 16 products per (cin, cout) instead of 36,
// i.e. 16 GEMMs (one per transform position xi = 4 i + j) of [cout x cin] x [cin x tile], 4/9 of the direct form's MFMAs.
//   B^T d along an axis: (d0 - d2, d1 + d2, d2 - d1, d1 - d3)             (y first, then x)
//   G g  along an axis: s = g0 + g2: (g0, 0.5 (s + g1), 0.5 (s - g1), g2)   (x first, then y)
//   A^T m along an axis: ((m0 + m1) + m2, (m1 - m2) - m3)                   (y first, then x)
// tools/winograd_numerics.py mirrors this operation order in fp32 (tests/test_winograd_numerics.py).
// Work split: the layer's 2x2 tiles form blocks of 16 (MFMA columns), its output channels blocks of 16 (MFMA rows); every wave runs NB
// (tile block, channel block) passes one after the other.  A pass walks K in groups of 16 input channels: lane (m, kq) reads the 4x4
// window of tile m for its four interleaved channels 16 G + 4 kq + e (16 ds_read_b128 from the direct loop's layouts) and transforms it
// in registers (V: 16 xi x 4 channels), loads U of cout m for the same channels (16 buffer loads, one per xi: U is a constant of the
// network, transformed once at pack time - NetLayout::w_wino, in the G g order above) and issues 16 xi x 4 k-steps.  The output
// transform is lane-local (the lane holds 4 couts x 16 xi of its tile): a pass ends with 16 floats per lane, so earlier passes' results wait in registers for the barrier in front of the in-place store at little cost.
// The transforms are written one scalar f32 add / mul at a time through wadd / wsub / wmul: left to itself the compiler SLP-packs
// neighbouring adds into v_pk_add_f32, which beside MFMAs costs more issue cycles than two plain adds.
__device__ __forceinline__ float wadd(float a, float b) { float r = a + b; asm("" : "+v"(r)); return r; }
__device__ __forceinline__ float wsub(float a, float b) { float r = a - b; asm("" : "+v"(r)); return r; }
__device__ __forceinline__ float wmul(float a, float b) { float r = a * b; asm("" : "+v"(r)); return r; }

// (tile row, tile column, channel block) of lane m's tile in pass q of `wave`
template <int H, int COUT, int NB>
__device__ __forceinline__ void wino_tile(int wave, int q, int m, int& ty, int& tx, int& cb) {
    constexpr int HT = H / 2, NCB = COUT / 16;
    const int p = wave * NB + q, tb = p / NCB;
    cb = p - tb * NCB;
    const int t = tb * 16 + m;
    ty = t / HT;
    tx = t - ty * HT;
}

// Weight operand of pass q of `wave`: byte offset of lane (cout m, kq) inside one (xi, K group) block [kq][cout][4] of the transformed weights
template <int H, int COUT, int NB>
__device__ __forceinline__ int wino_u_lane(int wave, int q, int lane) {
    int ty, tx, cb;
    wino_tile<H, COUT, NB>(wave, q, lane & 15, ty, tx, cb);
    return ((lane >> 4) * COUT + cb * 16 + (lane & 15)) * 16;
}

// U of K group G: one buffer_load_dwordx4 per transform position = the A operand of its four k-steps.  Wu = the packed U = G g G^T
// [xi][CIN/16][kq][COUT][4] (NetLayout::w_wino), computed once at pack time with the operation order above.  c: channel blocks past the lane's own
// (256 bytes = 16 couts each; the second block of a pair in conv3x3_wino_mfma_pair_rows)
template <int CIN, int COUT>
__device__ __forceinline__ f32x4 wino_load_u(__amdgpu_buffer_rsrc_t r, int u_lane, int k, int G, int c = 0) {
    return buf_read4(r, u_lane, (k * (CIN / 16) + G) * 16 * COUT * 4 + c * 256);
}

// U of the first K group of the wave's first pass: does not depend on the activations, so the kernel requests it BEFORE the barrier in
// front of the layer (what prefetch_b0 is to the direct loop).
template <int NW, int CIN, int COUT, int H, int NB>
__device__ __forceinline__ void wino_prefetch_u(const float* __restrict__ Wu, f32x4 (&U)[16], int wave, int lane) {
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(Wu, 16 * CIN * COUT);
    const int u_lane = wino_u_lane<H, COUT, NB>(wave, 0, lane);
#pragma unroll
    for (int k = 0; k < 16; ++k) U[k] = wino_load_u<CIN, COUT>(r, u_lane, k, 0);
}

// Position row i of V = B^T d B (xi = 4 i .. 4 i + 3) needs two rows of the window: B^T along y is t[c] = d[ra][c] -/+ d[rb][c] over the window rows
// (ra, rb) = (0, 2), (1, 2), (2, 1), (1, 3), a sum for i == 1 and a difference otherwise.
__device__ __forceinline__ constexpr int wino_row_a(int i) { return i == 0 ? 0 : (i == 2 ? 2 : 1); }
__device__ __forceinline__ constexpr int wino_row_b(int i) { return i == 2 ? 1 : (i == 3 ? 3 : 2); }

// The two window rows of position row i at LDS byte address `ab` of the window (8 ds_read_b128: the lane's four interleaved channels)
template <typename LI>
__device__ __forceinline__ void wino_read_rows(unsigned ab, int i, f32x4 (&da)[4], f32x4 (&db)[4]) {
    const int ra = wino_row_a(i), rb = wino_row_b(i);
#pragma unroll
    for (int c = 0; c < 4; ++c) { da[c] = lds_read4(ab + (ra * LI::WP + c) * 16); db[c] = lds_read4(ab + (rb * LI::WP + c) * 16); }
}

// The four V fragments V[0 .. 3] of position row i from its two window rows: B^T along y, then along x (32 VALU operations)
__device__ __forceinline__ void wino_transform_row(int i, const f32x4 (&da)[4], const f32x4 (&db)[4], f32x4* V) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] = i == 1 ? wadd(da[c][e], db[c][e]) : wsub(da[c][e], db[c][e]);
        V[0][e] = wsub(t[0], t[2]); V[1][e] = wadd(t[1], t[2]); V[2][e] = wsub(t[2], t[1]); V[3][e] = wsub(t[1], t[3]);
    }
}

// V = B^T d B of the 4x4 window at LDS byte address `ab` (16 ds_read_b128: the lane's four interleaved channels), along y, then along x: the arithmetic of
// wino_transform_row for all four rows at once, lane by lane (written as four calls it compiles to another instruction order in conv5 of HardNet:
// profiles/wino_helpers_report.md)
template <typename LI>
__device__ __forceinline__ void wino_window(unsigned ab, f32x4 (&V)[16]) {
    f32x4 d[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) d[r][c] = lds_read4(ab + (r * LI::WP + c) * 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t[4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            t[0][c] = wsub(d[0][c][e], d[2][c][e]); t[1][c] = wadd(d[1][c][e], d[2][c][e]);
            t[2][c] = wsub(d[2][c][e], d[1][c][e]); t[3][c] = wsub(d[1][c][e], d[3][c][e]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            V[4 * i][e] = wsub(t[i][0], t[i][2]); V[4 * i + 1][e] = wadd(t[i][1], t[i][2]);
            V[4 * i + 2][e] = wsub(t[i][2], t[i][1]); V[4 * i + 3][e] = wsub(t[i][1], t[i][3]);
        }
    }
}

// Y = A^T M A of the lane's 4 output channels x 16 positions: yq[2 dy + dx]
__device__ __forceinline__ void wino_output(const f32x4 (&acc)[16], f32x4 (&yq)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t[0][j] = wadd(wadd(acc[j][e], acc[4 + j][e]), acc[8 + j][e]);
            t[1][j] = wsub(wsub(acc[4 + j][e], acc[8 + j][e]), acc[12 + j][e]);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            yq[2 * r][e] = wadd(wadd(t[r][0], t[r][1]), t[r][2]);
            yq[2 * r + 1][e] = wsub(wsub(t[r][1], t[r][2]), t[r][3]);
        }
    }
}

// conv1 / conv3 of the exact HardNet trunk.  Pre-activation outputs (no bias) of the NB passes: y[q][2 dy + dx] = couts 16 cb + 4 (lane >> 4) + 0..3 of
// pixel (2 ty + dy, 2 tx + dx).  V = B^T d B does not depend on the output channel, and wino_tile gives passes 2 j and 2 j + 1 of a wave the same tile block
// and the channel blocks cb, cb + 1: the loop runs such a pair as ONE unit - one V against U of both channel blocks (the U address of cb + 1 is cb's plus
// 256 bytes) - so a window is transformed once per unit and not once per pass.  A unit walks rows as conv3x3_wino_mfma_rows does: a step is (unit, position
// row i, K group G), G fastest; it takes the two window rows of row i (8 ds_read_b128) and 32 VALU operations for the row's 4 V fragments and issues 2 x 4 x 4
// MFMAs into acc[2][4]; after the last G the row is folded into t0 / t1 of both channel blocks and after row 3 into y, operation by operation what
// wino_output does.  Every accumulator (tile, cout, position) receives the MFMAs of the one-pass-at-a-time form in its order (G ascending, four k-steps
// each, same operands), so the layer's bits do not change.  Rows 1 and 2 of a window are read twice per K group; with half as many windows the LDS reads
// are as many as before.
// Pipeline inside the wave: the reads and the transform of step s + 1 sit BETWEEN the 32 MFMAs of step s (sched_group_barrier: one read behind each of
// the first 8 MFMAs, two VALU behind each of the last 16 - the fp32 MFMA holds the pipe for 32 cycles and leaves the issue port to the VALU,
// tools/probes/mfma_valu_overlap.hip), in two V register sets Va / Vb that swap by name.  U enters holding step 0 (wino_prefetch_u_pair, requested in front
// of the barrier before the layer) and rolls one step ahead in its single set: fragment (c, k) of the next step is requested once the MFMAs of position k
// have issued, 24 MFMAs or more in front of its use.
template <int NW, int CIN, int COUT, int H, int NB>
__device__ __forceinline__ void wino_prefetch_u_pair(const float* __restrict__ Wu, f32x4 (&U)[2][4], int wave, int lane) {
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(Wu, 16 * CIN * COUT);
    const int u_lane = wino_u_lane<H, COUT, NB>(wave, 0, lane);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 2; ++c) U[c][k] = wino_load_u<CIN, COUT>(r, u_lane, k, 0, c);
}

template <int NW, int CIN, int COUT, typename LI, int NB>
__device__ __forceinline__ void conv3x3_wino_mfma_pair_rows(const float* act, const float* __restrict__ Wu, f32x4 (&U)[2][4], f32x4 (&y)[NB][4], int wave, int lane) {
    constexpr int H = LI::H, HT = H / 2, NGRP = CIN / 16, NSTEP = (NB / 2) * 4 * NGRP;
    static_assert(H % 2 == 0 && (HT * HT) % 16 == 0 && COUT % 16 == 0 && CIN % 16 == 0, "Winograd tiling");
    static_assert((HT * HT / 16) * (COUT / 16) == NW * NB, "the waves' passes must tile the layer exactly");
    static_assert(NB % 2 == 0 && (COUT / 16) % 2 == 0 && NSTEP % 2 == 0, "passes 2 j and 2 j + 1 must share their tile block");
    const int m = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wu, 16 * CIN * COUT);
    f32x4 t0[2][4], t1[2][4], acc[2][4], Va[4], Vb[4];
    auto window_addr = [&](int s) {
        const int u = s / (4 * NGRP), G = s % NGRP;
        int ty, tx, cb;
        wino_tile<H, COUT, NB>(wave, 2 * u, m, ty, tx, cb);
        unsigned ab = lds_byte_addr(act) + (((4 * G + kq) * LI::PSG + (2 * ty * LI::WP + 2 * tx) * 4) * 4);
        asm("" : "+v"(ab));
        return ab;
    };
    // one step: the MFMAs of step s on V, with the reads + transform of step s + 1 (into Vn) and the U requests of step s + 1 between them
    auto step = [&](int s, const f32x4 (&V)[4], f32x4 (&Vn)[4]) {
        const int u = s / (4 * NGRP), i = (s / NGRP) % 4, G = s % NGRP;
        const bool more = s + 1 < NSTEP;
        const int sn = more ? s + 1 : s;                  // (the last step re-requests its own weights: unused)
        const int un = sn / (4 * NGRP), in = (sn / NGRP) % 4, Gn = sn % NGRP;
        const int u_next = wino_u_lane<H, COUT, NB>(wave, 2 * un, lane);
        unsigned abn = 0;
        if (more) abn = window_addr(sn);
        if (G == 0) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[c][k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x4 da[4], db[4];
        if (more) wino_read_rows<LI>(abn, in, da, db);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {              // the two channel blocks' chains of position k interleave
                acc[0][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[0][k][s4], V[k][s4], acc[0][k], 0, 0, 0);   // U^T x V
                acc[1][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[1][k][s4], V[k][s4], acc[1][k], 0, 0, 0);
            }
            U[0][k] = wino_load_u<CIN, COUT>(wrsrc, u_next, 4 * in + k, Gn, 0);
            U[1][k] = wino_load_u<CIN, COUT>(wrsrc, u_next, 4 * in + k, Gn, 1);
        }
        if (more) {
            wino_transform_row(in, da, db, Vn);
            // pinned order: MFMAs 1 .. 8 each followed by one row read, U of position 0; MFMAs 9 .. 16, U of position 1; MFMAs 17 .. 32 each followed
            // by two operations of the transform (the reads have had 8 MFMAs or more to return), U of positions 2 and 3 behind MFMAs 24 and 32
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (G == NGRP - 1) {                               // the row's sums over K are complete: y stage of A^T M A, in wino_output's order
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (i == 0) t0[c][j][e] = acc[c][j][e];
                        else if (i == 1) { t0[c][j][e] = wadd(t0[c][j][e], acc[c][j][e]); t1[c][j][e] = acc[c][j][e]; }
                        else if (i == 2) { t0[c][j][e] = wadd(t0[c][j][e], acc[c][j][e]); t1[c][j][e] = wsub(t1[c][j][e], acc[c][j][e]); }
                        else t1[c][j][e] = wsub(t1[c][j][e], acc[c][j][e]);
                    }
                if (i == 3) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        y[2 * u + c][0][e] = wadd(wadd(t0[c][0][e], t0[c][1][e]), t0[c][2][e]);
                        y[2 * u + c][1][e] = wsub(wsub(t0[c][1][e], t0[c][2][e]), t0[c][3][e]);
                        y[2 * u + c][2][e] = wadd(wadd(t1[c][0][e], t1[c][1][e]), t1[c][2][e]);
                        y[2 * u + c][3][e] = wsub(wsub(t1[c][1][e], t1[c][2][e]), t1[c][3][e]);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    {
        f32x4 da[4], db[4];
        wino_read_rows<LI>(window_addr(0), 0, da, db);
        wino_transform_row(0, da, db, Va);
    }
#pragma unroll
    for (int s = 0; s < NSTEP; s += 2) {
        step(s, Va, Vb);
        step(s + 1, Vb, Va);
    }
}

// conv5 (one block of 16 tiles, NW channel blocks, NGRP == NW K groups): every wave would transform the same windows for all K groups.
// Instead wave w transforms K group w once and the workgroup shares V through LDS, [G][xi][kq][m][4] floats (1 KB contiguous per (G, xi):
// conflict-free both ways), written over the layer's input after a barrier (every wave has read its group by then, so the input is
// consumed).  The loop then has no VALU transform: V rolls through one register set like U (16 ds_read_b128 per group, as before).
// The caller owns NGRP * 4096 floats at `act`.
template <int NW, int CIN, int COUT, typename LI>
__device__ __forceinline__ void conv3x3_wino_mfma_shared_v(float* act, const float* __restrict__ Wu, f32x4 (&U)[16], f32x4 (&y)[1][4], int wave, int lane) {
    constexpr int NGRP = CIN / 16;
    static_assert(LI::H == 8 && COUT == 16 * NW && NGRP == NW, "one tile block, one channel block and one K group per wave");
    const int m = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wu, 16 * CIN * COUT);
    int ty, tx, cb;
    wino_tile<8, COUT, 1>(wave, 0, m, ty, tx, cb);
    const int u_lane = wino_u_lane<8, COUT, 1>(wave, 0, lane);
    f32x4 V[16];
    wino_window<LI>(lds_byte_addr(act) + ((wave * 4 + kq) * LI::PSG + (2 * ty * LI::WP + 2 * tx) * 4) * 4, V);
    __syncthreads();                                      // the whole input has been read
    const unsigned v0 = lds_byte_addr(act) + lane * 16;
#pragma unroll
    for (int k = 0; k < 16; ++k) *reinterpret_cast<f32x4*>(&act[((wave * 16 + k) * 64 + lane) * 4]) = V[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = lds_read4(v0 + k * 1024);
    f32x4 acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int G = 0; G < NGRP; ++G) {
        const int Gn = G == NGRP - 1 ? G : G + 1;         // (the last group re-requests itself: unused)
        unsigned vb = v0 + Gn * 16 * 1024;
        asm("" : "+v"(vb));
        __builtin_amdgcn_sched_barrier(0);                // pinned: two positions' chains interleave, their U and V reloads follow
#pragma unroll
        for (int k = 0; k < 16; k += 2) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k][s4], V[k][s4], acc[k], 0, 0, 0);
                acc[k + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k + 1][s4], V[k + 1][s4], acc[k + 1], 0, 0, 0);
            }
            U[k] = wino_load_u<CIN, COUT>(wrsrc, u_lane, k, Gn);
            U[k + 1] = wino_load_u<CIN, COUT>(wrsrc, u_lane, k + 1, Gn);
            V[k] = lds_read4(vb + k * 1024);
            V[k + 1] = lds_read4(vb + (k + 1) * 1024);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    wino_output(acc, y[0]);
}

// ---- Winograd F(4x4, 3x3): conv3 of the exact HardNet trunk in descriptor form 2 ----------------------------------------------------------
// A 4x4 output tile over its 6x6 input window, points 0, +-1, +-2: 36 products per (cin, cout) for 16 outputs, 2.25 per output against F(2x2, 3x3)'s 4.
//   B^T d along an axis: (4 d0 - 5 d2) + d4;  a = d4 - 4 d2, b = d3 - 4 d1: a + b, a - b;  c = d4 - d2, e = 2 (d3 - d1): c + e, c - e;  (4 d1 - 5 d3) + d5
//                                                                                                                               (y first, then x)
//   G g along an axis:   weights_layout.h: f43_g_axis                                                                           (x first, then y)
//   A^T m along an axis: p = m1 + m2, q = m1 - m2, r = m3 + m4, s = m3 - m4:  (m0 + p) + r,  q + 2 s,  p + 4 r,  q + (8 s + m5)    (x first, then y)
// tools/winograd_numerics.py: f43_conv3x3 mirrors this operation order in fp32.
// conv3 (64 -> 64 at 16 x 16) is ONE block of 16 tiles (tile m = (ty, tx) = (m >> 2, m & 3)), four channel blocks and four K groups; the layer runs as conv5's
// shared-V loop does, with a wave PAIR per channel block: wave w = 2 p + h
//   * transforms K group p for the position rows 3 h .. 3 h + 2 (xi = 6 i + j): lane (m, kq) reads rows h .. h + 4 of its window for its four interleaved channels
//     (30 ds_read_b128; the 16 windows of a service group lie 64 bytes and 4 rows apart and meet 4 at a time in the same banks - a 4-way conflict that no numbering of
//     the tiles removes, since it is the same set of addresses) and forms 18 V fragments; then barrier (the input is consumed), V into LDS as
//     [G][xi][kq][m][4] (1 KB contiguous per (G, xi): conflict-free both ways; 147 456 bytes over the layer's input), barrier;
//   * runs the 18 positions of its half against channel block p over the four K groups: 288 MFMAs into 18 accumulators, no VALU in the loop; U (a.wino_u: F43, derived
//     in front of the launch) and V roll one K group ahead, each in one register set, a position's fragments requested once its MFMAs have issued;
//   * folds its accumulators along x (f43_at_axis per position row) into t[3][4] and, in f43_combine, along y into its share of the four output rows, exchanges the
//     other half's share with its partner through LDS (8 KB per wave, fixed order, no atomics) and ends with y[4 dy + c] = pre-activation couts 16 p + 4 (lane >> 4) + 0..3
//     of pixel (4 ty + 2 h + dy, 4 tx + c).
// Every accumulator (tile, cout, position) receives its MFMAs in one fixed order (G ascending, four k-steps each).
struct F43L {                                             // float offsets from the start of the activation buffer
    static constexpr int V_FLOATS = 4 * F43_XI * 256;     // V of conv3: [G (4)][xi (36)][kq][m][4]
    static constexpr int X = 0, X_FLOATS = 8 * 8 * 256;   // the exchange slots of f43_combine, over V (dead behind the barrier in front of the combine)
};
__device__ __forceinline__ void f43_bt_lo(float d0, float d1, float d2, float d3, float d4, float& v0, float& v1, float& v2) {
    v0 = (4.0f * d0 - 5.0f * d2) + d4;
    const float a = d4 - 4.0f * d2, b = d3 - 4.0f * d1;
    v1 = a + b; v2 = a - b;
}
__device__ __forceinline__ void f43_bt_hi(float d1, float d2, float d3, float d4, float d5, float& v3, float& v4, float& v5) {
    const float c = d4 - d2, e = 2.0f * (d3 - d1);
    v3 = c + e; v4 = c - e;
    v5 = (4.0f * d1 - 5.0f * d3) + d5;
}
__device__ __forceinline__ void f43_at_axis(float m0, float m1, float m2, float m3, float m4, float m5, float& y0, float& y1, float& y2, float& y3) {
    const float p = m1 + m2, q = m1 - m2, r = m3 + m4, s = m3 - m4;
    y0 = (m0 + p) + r; y1 = q + 2.0f * s; y2 = p + 4.0f * r; y3 = q + (8.0f * s + m5);
}

// V[6 il + j] = position (3 HF + il, j) of B^T d B of the 6x6 window at LDS byte address `ab`, the lane's four interleaved channels: rows HF .. HF + 4 of the window
// (30 ds_read_b128), along y, then along x.  No MFMA runs beside it, so the arithmetic is plain C (the compiler may pack it)
template <typename LI, int HF>
__device__ __forceinline__ void f43_window_half(unsigned ab, f32x4 (&V)[18]) {
    f32x4 d[5][6];
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) d[r][c] = lds_read4(ab + ((r + HF) * LI::WP + c) * 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t[3][6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if constexpr (HF == 0) f43_bt_lo(d[0][c][e], d[1][c][e], d[2][c][e], d[3][c][e], d[4][c][e], t[0][c], t[1][c], t[2][c]);
            else f43_bt_hi(d[0][c][e], d[1][c][e], d[2][c][e], d[3][c][e], d[4][c][e], t[0][c], t[1][c], t[2][c]);
        }
#pragma unroll
        for (int il = 0; il < 3; ++il) {
            float v[6];
            f43_bt_lo(t[il][0], t[il][1], t[il][2], t[il][3], t[il][4], v[0], v[1], v[2]);
            f43_bt_hi(t[il][1], t[il][2], t[il][3], t[il][4], t[il][5], v[3], v[4], v[5]);
#pragma unroll
            for (int j = 0; j < 6; ++j) V[6 * il + j][e] = v[j];
        }
    }
}

// U of K group 0 of the wave's 18 positions: does not depend on the activations, requested in front of the barrier before the layer.  Wu = U of the layer,
// [xi (36)][CIN/16][kq][COUT][4]
template <int CIN, int COUT>
__device__ __forceinline__ int f43_u_lane(int wave, int lane) {
    return ((lane >> 4) * COUT + (wave >> 1) * 16 + (lane & 15)) * 16 + (wave & 1) * (18 * CIN * COUT * 4);
}
template <int CIN, int COUT>
__device__ __forceinline__ void f43_prefetch_u(const float* __restrict__ Wu, f32x4 (&U)[18], int wave, int lane) {
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(Wu, F43_XI * CIN * COUT);
    const int u_lane = f43_u_lane<CIN, COUT>(wave, lane);
#pragma unroll
    for (int k = 0; k < 18; ++k) U[k] = wino_load_u<CIN, COUT>(r, u_lane, k, 0);
}

// The caller owns F43L::V_FLOATS floats at `act`.  t[il][c] = the wave's position row 3 h + il folded along x (columns c = 0 .. 3 of the tile)
template <int NW, int CIN, int COUT, typename LI>
__device__ __forceinline__ void conv3x3_f43_mfma_shared_v(float* act, const float* __restrict__ Wu, f32x4 (&U)[18], f32x4 (&t)[3][4], int wave, int lane) {
    constexpr int NGRP = CIN / 16;
    static_assert(NW == 8 && LI::H == 16 && COUT == 16 * (NW / 2) && NGRP == NW / 2, "one block of 16 4x4 tiles; a wave pair per channel block and per K group");
    const int m = lane & 15, kq = lane >> 4, p = wave >> 1, h = wave & 1;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wu, F43_XI * CIN * COUT);
    const int u_lane = f43_u_lane<CIN, COUT>(wave, lane);
    f32x4 V[18];
    {
        const unsigned ab = lds_byte_addr(act) + ((4 * p + kq) * LI::PSG + (4 * (m >> 2) * LI::WP + 4 * (m & 3)) * 4) * 4;
        if (h == 0) f43_window_half<LI, 0>(ab, V); else f43_window_half<LI, 1>(ab, V);
    }
    __syncthreads();                                      // the whole input has been read
#pragma unroll
    for (int k = 0; k < 18; ++k) *reinterpret_cast<f32x4*>(&act[((p * F43_XI + 18 * h + k) * 64 + lane) * 4]) = V[k];
    __syncthreads();
    const unsigned v0 = lds_byte_addr(act) + (18 * h * 64 + lane) * 16;
#pragma unroll
    for (int k = 0; k < 18; ++k) V[k] = lds_read4(v0 + k * 1024);
    f32x4 acc[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int G = 0; G < NGRP; ++G) {
        const int Gn = G == NGRP - 1 ? G : G + 1;         // (the last group re-requests itself: unused.  Peeling it so that it requests nothing was measured: the
                                                          // layer 29.70 k -> 29.37 k ticks, inside the run-to-run noise of the headline; not kept)
        unsigned vb = v0 + Gn * F43_XI * 1024;
        asm("" : "+v"(vb));
        __builtin_amdgcn_sched_barrier(0);                // pinned: two positions' chains interleave, their U and V reloads follow
#pragma unroll
        for (int k = 0; k < 18; k += 2) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k][s4], V[k][s4], acc[k], 0, 0, 0);
                acc[k + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k + 1][s4], V[k + 1][s4], acc[k + 1], 0, 0, 0);
            }
            U[k] = wino_load_u<CIN, COUT>(wrsrc, u_lane, k, Gn);
            U[k + 1] = wino_load_u<CIN, COUT>(wrsrc, u_lane, k + 1, Gn);
            V[k] = lds_read4(vb + k * 1024);
            V[k + 1] = lds_read4(vb + (k + 1) * 1024);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int il = 0; il < 3; ++il)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float yc[4];
            f43_at_axis(acc[6 * il][e], acc[6 * il + 1][e], acc[6 * il + 2][e], acc[6 * il + 3][e], acc[6 * il + 4][e], acc[6 * il + 5][e], yc[0], yc[1], yc[2], yc[3]);
#pragma unroll
            for (int c = 0; c < 4; ++c) t[il][c][e] = yc[c];
        }
}

// A^T along y over the wave pair, f43_at_axis's sums: wave 2 p (rows m0, m1, m2 = t[0 .. 2]) forms p, q and m0 + p, wave 2 p + 1 (m3, m4, m5) forms r, 2 s, 4 r and
// 8 s + m5; wave 2 p sends p and q, wave 2 p + 1 sends r and 2 s (8 fragments each into its 8 KB slot of F43L::X), barrier, and wave 2 p ends with the tile's output
// rows 0 and 1, wave 2 p + 1 with rows 2 and 3.  The caller has passed a barrier behind the loop (X lies over V) and passes another before anything is stored over X.
// `lds` = the start of the activation buffer
__device__ __forceinline__ void f43_combine(float* lds, const f32x4 (&t)[3][4], f32x4 (&y)[8], int wave, int lane) {
    const int h = wave & 1;
    float* xw = lds + F43L::X + (wave * 8 * 64 + lane) * 4;
    const float* xr = lds + F43L::X + ((wave ^ 1) * 8 * 64 + lane) * 4;
    f32x4 k0[4], k1[4];                                   // what the wave keeps: (m0 + p, q) or (4 r, 8 s + m5)
    if (h == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x4 p = t[1][c] + t[2][c], q = t[1][c] - t[2][c];
            k0[c] = t[0][c] + p; k1[c] = q;
            *reinterpret_cast<f32x4*>(&xw[c * 256]) = p;
            *reinterpret_cast<f32x4*>(&xw[(4 + c) * 256]) = q;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x4 r = t[0][c] + t[1][c], s = t[0][c] - t[1][c];
            k0[c] = 4.0f * r; k1[c] = 8.0f * s + t[2][c];
            *reinterpret_cast<f32x4*>(&xw[c * 256]) = r;
            *reinterpret_cast<f32x4*>(&xw[(4 + c) * 256]) = 2.0f * s;
        }
    }
    __syncthreads();                                      // the partner's share is in place
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const f32x4 o0 = *reinterpret_cast<const f32x4*>(&xr[c * 256]), o1 = *reinterpret_cast<const f32x4*>(&xr[(4 + c) * 256]);
        y[c] = k0[c] + o0;                                // rows 0 / 2: (m0 + p) + r, p + 4 r
        y[4 + c] = k1[c] + o1;                            // rows 1 / 3: q + 2 s, q + (8 s + m5)
    }
}

// + bias, ReLU, store the wave's 2 x 4 pixels x 4 channels per lane into the LDS layout LO (H = 16)
template <typename LO>
__device__ __forceinline__ void f43_store_lds(float* act, f32x4 bias, const f32x4 (&y)[8], int wave, int lane) {
    const int m = lane & 15, oy = 4 * (m >> 2) + 2 * (wave & 1), ox = 4 * (m & 3);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const f32x4 v = bias_relu(y[k], bias);
        *reinterpret_cast<f32x4*>(&act[((wave >> 1) * 4 + (lane >> 4)) * LO::PSG + ((oy + (k >> 2) + 1) * LO::WP + ox + (k & 3) + 1) * 4]) = v;
    }
}

// ---- conv5 of HardNet's descriptor form 3: F(4x4, 3x3) over FOUR patches per workgroup (hardnet_conv5_f43.hip: hardnet_conv5_f43_kernel) ----------------------
// conv5 (128 -> 128 at 8 x 8) has four 4x4 tiles per patch; four consecutive patches fill the MFMA's 16 columns, m = 4 patch + 2 ty + tx.  Wave w owns channel block w,
// all 36 positions and all of K: 36 accumulators live over the whole layer, no exchange between waves (no f43_combine).  K runs in four quarters of 32 channels (two K
// groups): a quarter's input, global [c / 4][pixel][4] per patch (wino_store_global_c4), goes into a zero-haloed 10 x 10 LDS tile per (patch, channel group); thread
// (channel group, m, e) transforms ONE channel of one window (f43_bt_lo / f43_bt_hi along y, then x: f43_window_half's operations) into V [G (2)][xi][kq][m][4]; then every wave
// runs 2 x 36 positions x 4 k-steps with no VALU in the loop.  The next quarter's input is requested in front of the transform and lands under the loop.
struct F43C5L {                                           // float offsets in the kernel's LDS
    static constexpr int WPI = 10;                        // row of the padded input tile
    static constexpr int CGS = WPI * WPI * 4;             // a channel group (4 interleaved channels) of a patch
    static constexpr int PS = 8 * CGS + 4;                // a patch: the quarter's 8 channel groups, + 4 floats: the transform's ds_read_b32 of 4 patches x 2 tx x 4 channels cover the 32 banks
    static constexpr int IN = 0, IN_FLOATS = 4 * PS;
    static constexpr int V = IN_FLOATS, V_FLOATS = 2 * F43_XI * 256;
    static constexpr int TOTAL = V + V_FLOATS;            // 124 992 bytes
};
static_assert(F43C5L::V % 4 == 0 && F43C5L::PS % 4 == 0 && F43C5L::TOTAL * 4 <= 160 * 1024, "16-byte aligned sections within the CU's LDS");

// One channel of one 6x6 window at `in` (floats, row pitch WPI * 4, column pitch 4) -> its 36 positions, position xi at v[xi * XS]: B^T d B along y, then along x
template <int WPI, int XS>
__device__ __forceinline__ void f43_transform_channel(const float* in, float* v) {
    float t[6][6];                                        // t[i][c]
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        float d[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) d[r] = in[(r * WPI + c) * 4];
        f43_bt_lo(d[0], d[1], d[2], d[3], d[4], t[0][c], t[1][c], t[2][c]);
        f43_bt_hi(d[1], d[2], d[3], d[4], d[5], t[3][c], t[4][c], t[5][c]);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float o[6];
        f43_bt_lo(t[i][0], t[i][1], t[i][2], t[i][3], t[i][4], o[0], o[1], o[2]);
        f43_bt_hi(t[i][1], t[i][2], t[i][3], t[i][4], t[i][5], o[3], o[4], o[5]);
#pragma unroll
        for (int j = 0; j < 6; ++j) v[(6 * i + j) * XS] = o[j];
    }
}
__device__ __forceinline__ void f43c5_transform(const float* in, float* v) { f43_transform_channel<F43C5L::WPI, 256>(in, v); }

// Y = A^T M A of the lane's 4 output channels (x first, then y: f43_at_axis both ways, the sums f43_combine forms over a wave pair): y[4 dy + c]
__device__ __forceinline__ void f43c5_output(const f32x4 (&acc)[F43_XI], f32x4 (&y)[16]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t[6][4];
#pragma unroll
        for (int i = 0; i < 6; ++i) f43_at_axis(acc[6 * i][e], acc[6 * i + 1][e], acc[6 * i + 2][e], acc[6 * i + 3][e], acc[6 * i + 4][e], acc[6 * i + 5][e], t[i][0], t[i][1], t[i][2], t[i][3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float yr[4];
            f43_at_axis(t[0][c], t[1][c], t[2][c], t[3][c], t[4][c], t[5][c], yr[0], yr[1], yr[2], yr[3]);
#pragma unroll
            for (int dy = 0; dy < 4; ++dy) y[4 * dy + c][e] = yr[dy];
        }
    }
}

// ---- conv0 + conv1 of HardNet's descriptor form 4: conv1 as F(4x4, 3x3), the layer pair streamed over conv1's K (cnn_trunk.h: the STREAM1 block) ----------------
// conv1 (32 -> 32 at 32 x 32) has 64 4x4 tiles = four blocks of 16 (tile t = 8 ty + tx, block t >> 4 = two tile rows, m = t & 15) and two channel blocks; wave w owns
// (tile block w >> 1, channel block w & 1), all 36 positions and all of K: 36 accumulators live over the whole layer, no exchange between waves.  V of the layer would be
// 295 KB, and conv0's output fills the activation buffer - but conv0 reads only the resident patch, so it runs ONE channel block (= one K group of conv1) at a time into a
// half-size layout, and a K group runs in two quarters of 8 channels: k-steps 2 jh and 2 jh + 1 = channels 16 G + 4 kq + 2 jh + {0, 1}, the .xy / .zw of U's float4.
// Per quarter thread (tile, kq, j) transforms ONE channel of one window (f43_transform_channel) into V [xi][tile block][slot(kq, m)][2]; then every wave runs 36 positions x
// 2 k-steps with no VALU in the loop: U as 8-byte buffer loads, V as one ds_read_b64 per position (512 bytes contiguous per wave).
// Banks (32 for ds_read_b32 and every ds_write, per 32-lane half; tests/test_winograd_f43_conv1_numerics.py runs the model): a half of the transform = (j, kq, tx & 3).  Its
// window reads hit j + 4 kq + 16 (tx & 1): 16 banks, 2-way - a quarter reads half of every 16-byte cell, so no group stride does better; GS = 4 (mod 32) reaches the 16.  Its
// V stores would meet 4-way in [kq][m][2] (kq is 64 floats apart), so the 16 m of a kq are rotated by 4 kq: slot = 16 kq + ((m + 4 kq) & 15), conflict-free for the
// stores and, a rotation within 128 bytes, for the loop's ds_read_b64 as well.
struct F43C1L {                                           // float offsets from the start of the activation buffer
    static constexpr int GS = 4676;                       // group stride of conv0's half output [kq][padded pixel 34 x 34][4]
    static constexpr int C0_FLOATS = 4 * GS;
    static constexpr int XS = 4 * 64 * 2;                 // a position of V: four tile blocks x 64 slots x 2 channels
    static constexpr int V = C0_FLOATS, V_FLOATS = F43_XI * XS;
    static constexpr int TOTAL = V + V_FLOATS;            // 148 544 bytes
    __device__ static __forceinline__ int slot(int kq, int m) { return 16 * kq + ((m + 4 * kq) & 15); }
};
typedef Lay<32, 34, F43C1L::GS> LayS1;                    // conv0's half output -> the quarter transforms
static_assert(F43C1L::TOTAL <= 8 * LayC0::PSG && 8 * LayC1::PSG <= 8 * LayC0::PSG && F43C1L::V % 4 == 0 && F43C1L::GS % 32 == 4, "the pair fits the activation buffer, 16-byte aligned");

// conv0 of ONE channel tile (16 channels) into LayS1: conv0_mfma's chain for every value (accumulator = bias, then the taps in three MFMAs) and store_tiles_lds's ReLU and
// address, but each of the wave's eight pixel tiles is stored as soon as it is complete - the 144 accumulators of conv1 are live beside it, 4 registers here instead of 32.
// b = the lane's taps of the channel tile (conv0_load_w's b[.][tile]), bv = its bias
__device__ __forceinline__ void f43c1_conv0_tile(const float* patch, const float (&b)[3], f32x4 bv, float* act, int wave, int lane) {
    const int m = lane & 15, kq = lane >> 4;
    int toff[3];
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3) {
        const int t = 4 * s3 + kq;
        toff[s3] = t < 9 ? (t / 3) * WP32 + (t % 3) : 0;              // taps 9..11: any valid address (weight is zero)
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = (wave * 8 + i) * 16 + m, oy = p >> 5, ox = p & 31;
        f32x4 acc = bv;
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b[s3], patch[oy * WP32 + ox + toff[s3]], acc, 0, 0, 0);
        *reinterpret_cast<f32x4*>(&act[kq * LayS1::PSG + ((oy + 1) * LayS1::WP + ox + 1) * 4]) = relu4(acc);
    }
}

typedef __attribute__((address_space(3))) const f32x2 LdsF2;
__device__ __forceinline__ f32x2 lds_read2(unsigned byte_addr) { return *(LdsF2*)(size_t)byte_addr; }
// U of position k, the two k-steps of a quarter: `q_off` = the quarter's byte offset inside a position's block, G * 16 * COUT * 4 + 8 jh
template <int CIN, int COUT>
__device__ __forceinline__ f32x2 f43c1_load_u(__amdgpu_buffer_rsrc_t r, int u_lane, int k, int q_off) {
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, u_lane, k * (CIN / 16) * 16 * COUT * 4 + q_off, 0));
}
// One quarter's loop: 36 positions x 2 k-steps.  U enters holding positions 0 .. DU - 1 of this quarter and leaves holding those of the next (q_next; the last quarter
// re-requests itself: unused); V (v0: positions 0 .. 17, v1: 18 .. 35 - a position is 2 KB, the DS offset field ends at 64 KB) rolls DV positions ahead within the quarter.
template <int CIN, int COUT, int DU, int DV>
__device__ __forceinline__ void f43c1_quarter_loop(__amdgpu_buffer_rsrc_t wrsrc, int u_lane, int q_off, int q_next, unsigned v0, unsigned v1, f32x2 (&Ur)[DU], f32x4 (&acc)[F43_XI]) {
    static_assert(F43_XI % DU == 0 && F43_XI % DV == 0 && DU % 2 == 0 && DV % 2 == 0 && DV <= 18, "the sets roll with compile-time indices");
    f32x2 Vr[DV];
#pragma unroll
    for (int k = 0; k < DV; ++k) Vr[k] = lds_read2(v0 + k * (F43C1L::XS * 4));
    __builtin_amdgcn_sched_barrier(0);                    // pinned: two positions' chains interleave, their U and V reloads follow
#pragma unroll
    for (int k = 0; k < F43_XI; k += 2) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ur[k % DU][s], Vr[k % DV][s], acc[k], 0, 0, 0);
            acc[k + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ur[(k + 1) % DU][s], Vr[(k + 1) % DV][s], acc[k + 1], 0, 0, 0);
        }
#pragma unroll
        for (int kk = k; kk < k + 2; ++kk) {
            const int ku = kk + DU, kv = kk + DV;
            Ur[kk % DU] = ku < F43_XI ? f43c1_load_u<CIN, COUT>(wrsrc, u_lane, ku, q_off) : f43c1_load_u<CIN, COUT>(wrsrc, u_lane, ku - F43_XI, q_next);
            if (kv < F43_XI) Vr[kk % DV] = kv < 18 ? lds_read2(v0 + kv * (F43C1L::XS * 4)) : lds_read2(v1 + (kv - 18) * (F43C1L::XS * 4));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// + bias, ReLU, store the lane's 4 x 4 pixels x 4 channels (f43c5_output's y) into the LDS layout LO (H = 32)
template <typename LO>
__device__ __forceinline__ void f43c1_store_lds(float* act, f32x4 bias, const f32x4 (&y)[16], int wave, int lane) {
    const int t = (wave >> 1) * 16 + (lane & 15), oy = 4 * (t >> 3), ox = 4 * (t & 7);
    float* dst = act + ((wave & 1) * 4 + (lane >> 4)) * LO::PSG + ((oy + 1) * LO::WP + ox + 1) * 4;
#pragma unroll
    for (int k = 0; k < 16; ++k) *reinterpret_cast<f32x4*>(dst + ((k >> 2) * LO::WP + (k & 3)) * 4) = bias_relu(y[k], bias);
}

// The same layer for the 16-channel trunks (AffNet / OriNet conv1, conv3), which live on 128 registers per lane (two workgroups per CU): acc[16] + U[16] +
// V[16] of a whole-window loop do not fit.  The output transform is linear in the positions, so a wave walks ONE ROW of four positions xi = 4 i .. 4 i + 3 at a
// time: row i of V needs two rows of the window (B^T along y: rows (0, 2), (1, 2), (2, 1), (1, 3)), 8 ds_read_b128 and 32 VALU operations; the row's four
// accumulators run over all K groups (same K order per position as every Winograd loop here: G ascending, four k-steps each) and are then folded into the y stage of
// A^T M A - t0 = (m0 + m1) + m2, t1 = (m1 - m2) - m3, operation by operation what wino_output does - before the next row starts.  Live: 4 accumulators, 4 U
// fragments, 4 V fragments, t0 / t1.  Per K group the window rows 1 and 2 are read twice (32 instead of 16 ds_read_b128), the VALU work is the same.
// U enters holding row 0 / group 0 of pass 0 (wino_prefetch_u_row) and rolls one step ahead in its single register set.
// Wu = U of the layer, [xi][CIN/16][kq][COUT][4], derived on the device from the blob's taps (derive_u.hip: derive_u_kernel).
template <int NW, int CIN, int COUT, int H, int NB>
__device__ __forceinline__ void wino_prefetch_u_row(const float* __restrict__ Wu, f32x4 (&U)[4], int wave, int lane) {
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(Wu, 16 * CIN * COUT);
    const int u_lane = wino_u_lane<H, COUT, NB>(wave, 0, lane);
#pragma unroll
    for (int k = 0; k < 4; ++k) U[k] = wino_load_u<CIN, COUT>(r, u_lane, k, 0);
}

template <int NW, int CIN, int COUT, typename LI, int NB>
__device__ __forceinline__ void conv3x3_wino_mfma_rows(const float* act, const float* __restrict__ Wu, f32x4 (&U)[4], f32x4 (&y)[NB][4], int wave, int lane) {
    constexpr int H = LI::H, HT = H / 2, NGRP = CIN / 16, NSTEP = NB * 4 * NGRP;
    static_assert(H % 2 == 0 && (HT * HT) % 16 == 0 && COUT % 16 == 0 && CIN % 16 == 0, "Winograd tiling");
    static_assert((HT * HT / 16) * (COUT / 16) == NW * NB, "the waves' passes must tile the layer exactly");
    const int m = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wu, 16 * CIN * COUT);
    f32x4 t0[4], t1[4], acc[4];
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {                     // step = (pass q, position row i, K group G), G fastest
        const int q = s / (4 * NGRP), i = (s / NGRP) % 4, G = s % NGRP;
        const int sn = s + 1 < NSTEP ? s + 1 : s;         // (the last step re-requests its own weights: unused)
        const int qn = sn / (4 * NGRP), in = (sn / NGRP) % 4, Gn = sn % NGRP;
        int ty, tx, cb;
        wino_tile<H, COUT, NB>(wave, q, m, ty, tx, cb);
        const int u_next = wino_u_lane<H, COUT, NB>(wave, qn, lane);
        unsigned ab = lds_byte_addr(act) + (((4 * G + kq) * LI::PSG + (2 * ty * LI::WP + 2 * tx) * 4) * 4);
        asm("" : "+v"(ab));
        f32x4 da[4], db[4], V[4];
        wino_read_rows<LI>(ab, i, da, db);
        wino_transform_row(i, da, db, V);
        if (G == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_sched_barrier(0);                // pinned: two positions' chains interleave, their U reloads follow
#pragma unroll
        for (int k = 0; k < 4; k += 2) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k][s4], V[k][s4], acc[k], 0, 0, 0);   // U^T x V
                acc[k + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k + 1][s4], V[k + 1][s4], acc[k + 1], 0, 0, 0);
            }
            U[k] = wino_load_u<CIN, COUT>(wrsrc, u_next, 4 * in + k, Gn);
            U[k + 1] = wino_load_u<CIN, COUT>(wrsrc, u_next, 4 * in + k + 1, Gn);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (G == NGRP - 1) {                               // the row's sums over K are complete: y stage of A^T M A, in wino_output's order
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (i == 0) t0[j][e] = acc[j][e];
                    else if (i == 1) { t0[j][e] = wadd(t0[j][e], acc[j][e]); t1[j][e] = acc[j][e]; }
                    else if (i == 2) { t0[j][e] = wadd(t0[j][e], acc[j][e]); t1[j][e] = wsub(t1[j][e], acc[j][e]); }
                    else t1[j][e] = wsub(t1[j][e], acc[j][e]);
                }
            if (i == 3) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    y[q][0][e] = wadd(wadd(t0[0][e], t0[1][e]), t0[2][e]);
                    y[q][1][e] = wsub(wsub(t0[1][e], t0[2][e]), t0[3][e]);
                    y[q][2][e] = wadd(wadd(t1[0][e], t1[1][e]), t1[2][e]);
                    y[q][3][e] = wsub(wsub(t1[1][e], t1[2][e]), t1[3][e]);
                }
            }
        }
    }
}

// conv5 of the exact OriNet trunk (64 -> 64 @8x8): one block of 16 tiles, four channel blocks, four K groups, 1024 MFMAs = 128 per wave.  Wave w = 2 p + h
// runs channel block p on the position rows 2 h and 2 h + 1 over all four K groups, as conv3x3_wino_mfma_rows walks its rows: a step is (position row, K
// group), G fastest (the K order of every Winograd loop here), 8 ds_read_b128 + 32 VALU operations for the row's four V fragments, 16 MFMAs; U rolls one step
// ahead in its single set and enters holding step 0 (wino5_prefetch_u).  (V is NOT shared through LDS as in HardNet's conv5: V of the layer is 16 positions x 64
// channels x 16 tiles = 64 KB, which neither fits beside conv4's 43 KB output nor leaves room for the exchange below - sharing would cost three more barriers
// per patch.)
// Combine (wino5_combine), in wino_output's operation order: the y stage of A^T M A is t0 = (m0 + m1) + m2, t1 = (m1 - m2) - m3 over the position rows m_i.
// Wave 2 p holds m0, m1 and wave 2 p + 1 holds m2, m3: wave 2 p writes m1 and wave 2 p + 1 writes m2 to its 4 KB slot of Wino5::X, barrier, then wave 2 p forms
// t0 = (m0 + m1) + m2 and from it output row dy = 0, wave 2 p + 1 forms t1 = (m1 - m2) - m3 and output row dy = 1.  Fixed for every patch and launch, no atomics;
// the sums are those of wino_output (tools/winograd_numerics.py: wino_conv3x3).  X lies behind conv4's output, which other waves still read when a wave
// writes its slot, and runs past the activation buffer into the input patch and the reduction slots, both dead since conv0; after the barrier conv4's output is
// dead and takes the head's copy (Wino5::HEAD), clear of X, which the partner still reads.
// Result: y[dx] = pre-activation couts 16 p + 4 (lane >> 4) + 0..3 of pixel (2 ty + h, 2 tx + dx), tile (ty, tx) = (m >> 2, m & 3).
struct Wino5 {                                            // float offsets from the start of the activation buffer
    static constexpr int X = 16 * LayC4::PSG, X_FLOATS = 8 * 4 * 256;
    static constexpr int HEAD = 0;
    static constexpr int U_HALF = 8 * 4 * 16 * 64 * 4;    // bytes of U between positions xi and xi + 8
};
__device__ __forceinline__ void wino5_prefetch_u(const float* __restrict__ Wu, f32x4 (&U)[4], int wave, int lane) {
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(Wu, 16 * 64 * 64);
    const int u_lane = ((lane >> 4) * 64 + (wave >> 1) * 16 + (lane & 15)) * 16 + (wave & 1) * Wino5::U_HALF;
#pragma unroll
    for (int k = 0; k < 4; ++k) U[k] = wino_load_u<64, 64>(r, u_lane, k, 0);
}

template <int NW, typename LI>
__device__ __forceinline__ void conv3x3_wino_mfma_half_rows(const float* act, const float* __restrict__ Wu, f32x4 (&U)[4], f32x4 (&acc)[2][4], int wave, int lane) {
    constexpr int CIN = 64, COUT = 64, NGRP = CIN / 16, NSTEP = 2 * NGRP;
    static_assert(NW == 8 && LI::H == 8, "one tile block; a wave pair per channel block");
    const int m = lane & 15, kq = lane >> 4, p = wave >> 1;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wu, 16 * CIN * COUT);
    const int u_lane = (kq * COUT + p * 16 + m) * 16;
    const unsigned a0 = lds_byte_addr(act) + ((kq * LI::PSG + (2 * (m >> 2) * LI::WP + 2 * (m & 3)) * 4) * 4);
    auto rows = [&](auto hc) {                            // the loop of the wave's half: position rows 2 H2 and 2 H2 + 1 are compile-time constants
        constexpr int H2 = decltype(hc)::v;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {                 // step = (position row i, K group G), G fastest
            const int il = s / NGRP, i = 2 * H2 + il, G = s % NGRP;
            const int sn = s + 1 < NSTEP ? s + 1 : s;     // (the last step re-requests its own weights: unused)
            const int in = 2 * H2 + sn / NGRP, Gn = sn % NGRP;
            unsigned ab = a0 + 4 * G * LI::PSG * 4;
            asm("" : "+v"(ab));
            f32x4 da[4], db[4], V[4];
            wino_read_rows<LI>(ab, i, da, db);
            wino_transform_row(i, da, db, V);
            if (G == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[il][k] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            __builtin_amdgcn_sched_barrier(0);            // pinned: two positions' chains interleave, their U reloads follow
#pragma unroll
            for (int k = 0; k < 4; k += 2) {
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    acc[il][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k][s4], V[k][s4], acc[il][k], 0, 0, 0);
                    acc[il][k + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k + 1][s4], V[k + 1][s4], acc[il][k + 1], 0, 0, 0);
                }
                U[k] = wino_load_u<CIN, COUT>(wrsrc, u_lane, 4 * in + k, Gn);
                U[k + 1] = wino_load_u<CIN, COUT>(wrsrc, u_lane, 4 * in + k + 1, Gn);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    if ((wave & 1) == 0) rows(IntC<0>{}); else rows(IntC<1>{});
}

// `lds` = the start of the activation buffer
__device__ __forceinline__ void wino5_combine(float* lds, const f32x4 (&acc)[2][4], f32x4 (&y)[2], int wave, int lane) {
    const int h = wave & 1;
    float* xw = lds + Wino5::X + (wave * 4 * 64 + lane) * 4;
    const float* xr = lds + Wino5::X + ((wave ^ 1) * 4 * 64 + lane) * 4;
    if (h == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(&xw[j * 256]) = acc[1][j];       // m1
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(&xw[j * 256]) = acc[0][j];       // m2
    }
    __syncthreads();                                      // the partner's row is in place; every wave has finished reading conv4's output
    f32x4 o[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = *reinterpret_cast<const f32x4*>(&xr[j * 256]);
    if (h == 0) {                                         // t0 = (m0 + m1) + m2
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) t[j][e] = wadd(wadd(acc[0][j][e], acc[1][j][e]), o[j][e]);
    } else {                                              // t1 = (m1 - m2) - m3
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) t[j][e] = wsub(wsub(o[j][e], acc[0][j][e]), acc[1][j][e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        y[0][e] = wadd(wadd(t[0][e], t[1][e]), t[2][e]);
        y[1][e] = wsub(wsub(t[1][e], t[2][e]), t[3][e]);
    }
}

// + bias, ReLU, store the wave's two pixels x 4 channels per lane: pixel (oy, ox), channel c at dst[(oy * ROW + ox) * PIX + (c / 4) * GRP + c % 4]
// (a Lay layout: ROW = WP, PIX = 4, GRP = PSG, dst at its pixel (0, 0); the OriNet head copy: ROW = 10, PIX = ORI_HP, GRP = 4)
template <int ROW, int PIX, int GRP>
__device__ __forceinline__ void wino5_store_lds(float* dst, f32x4 bias, const f32x4 (&y)[2], int wave, int lane) {
    const int m = lane & 15, oy = 2 * (m >> 2) + (wave & 1), ox = 2 * (m & 3);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const f32x4 v = bias_relu(y[k], bias);
        *reinterpret_cast<f32x4*>(&dst[(oy * ROW + ox + k) * PIX + ((wave >> 1) * 4 + (lane >> 4)) * GRP]) = v;
    }
}

// bias of the lane's four output channels in each pass
template <int NW, int H, int COUT, int NB>
__device__ __forceinline__ void wino_bias(const float* __restrict__ bias, f32x4 (&bv)[NB], int wave, int lane) {
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        int ty, tx, cb;
        wino_tile<H, COUT, NB>(wave, q, lane & 15, ty, tx, cb);
        bv[q] = *reinterpret_cast<const f32x4*>(&bias[cb * 16 + 4 * (lane >> 4)]);
    }
}

// + bias, ReLU, store the 2x2 pixels x 4 channels of every pass into the LDS layout LO (H = LO::H, one ds_write_b128 per pixel)
template <int COUT, typename LO, int NB>
__device__ __forceinline__ void wino_store_lds(float* act, const f32x4 (&bias)[NB], const f32x4 (&y)[NB][4], int wave, int lane) {
    const int g = lane >> 4;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        int ty, tx, cb;
        wino_tile<LO::H, COUT, NB>(wave, q, lane & 15, ty, tx, cb);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int oy = 2 * ty + (k >> 1), ox = 2 * tx + (k & 1);
            const f32x4 v = bias_relu(y[q][k], bias[q]);
            *reinterpret_cast<f32x4*>(&act[(cb * 4 + g) * LO::PSG + ((oy + 1) * LO::WP + ox + 1) * 4]) = v;
        }
    }
}

// Same for HardNet's last trunk layer: global [pixel p][channel c] (store_tiles_global's order)
template <int COUT, int H, int NB>
__device__ __forceinline__ void wino_store_global(float* __restrict__ dst, const f32x4 (&bias)[NB], const f32x4 (&y)[NB][4], int wave, int lane) {
    const int g = lane >> 4;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        int ty, tx, cb;
        wino_tile<H, COUT, NB>(wave, q, lane & 15, ty, tx, cb);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = (2 * ty + (k >> 1)) * H + 2 * tx + (k & 1);
            const f32x4 v = bias_relu(y[q][k], bias[q]);
            *reinterpret_cast<f32x4*>(dst + p * COUT + cb * 16 + 4 * g) = v;
        }
    }
}

// Same for conv4 of HardNet's descriptor form 3: global [c / 4][pixel p][4], wino_store_lds's layout without the halo (hardnet_conv5_f43_kernel reads it back)
template <int COUT, int H, int NB>
__device__ __forceinline__ void wino_store_global_c4(float* __restrict__ dst, const f32x4 (&bias)[NB], const f32x4 (&y)[NB][4], int wave, int lane) {
    const int g = lane >> 4;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        int ty, tx, cb;
        wino_tile<H, COUT, NB>(wave, q, lane & 15, ty, tx, cb);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = (2 * ty + (k >> 1)) * H + 2 * tx + (k & 1);
            const f32x4 v = bias_relu(y[q][k], bias[q]);
            *reinterpret_cast<f32x4*>(dst + ((cb * 4 + g) * (H * H) + p) * 4) = v;
        }
    }
}

// ---- polyphase Winograd F(2x2, 2x2): the stride-2 layers of the exact HardNet trunk in form 1 (conv2, conv4) ------------------------------
// A 3x3 stride-2 padding-1 layer over 2x2 output tiles: along an axis the tile's outputs read the 5 input samples d0 .. d4, taps 0 and 2 on d0, d2, d4 (a
// 2-tap stride-1 filter, run as F(2, 2)) and tap 1 on d1, d3:
//   input   (d0 - d2, d2, d2 - d4 | d1, d3)                      (y first, then x)
//   weight  (g0, g0 + g2, g2 | g1, g1)                           (x first, then y; weights_layout.h: poly_weight_transform)
//   output  ((m0 + m1) + n0, (m1 - m2) + n1)                     (y first, then x)
// 25 products per (cin, cout, tile) instead of 36: position rows 0 .. 2 (odd window rows x odd columns, 3 positions each, xi = 3 i + j), 3 .. 5 (odd rows x
// even columns, 2 each, xi = 9 + 2 i + j), 6 .. 7 (even rows x odd columns, xi = 15 + 3 i + j), 8 .. 9 (even x even, xi = 21 + 2 i + j).
// tools/winograd_numerics.py: poly_conv3x3_s2 mirrors the operation order.
// The loop is conv3x3_wino_mfma_pair_rows' with rows of 3 or 2 positions: a unit is one block of 16 tiles against NCB channel blocks (2: one V against U of both;
// 1: conv4, whose eight waves share the one tile block); a step is (unit, position row, K group), G fastest; it reads the one or two window rows of its position
// row at the 3 or 2 columns of its phase (2 .. 6 ds_read_b128), transforms them (0 .. 20 VALU operations) and issues NP x 4 x NCB MFMAs; after the last G the row's
// accumulators fold into the y stage (t0 / t1, five columns each).  Every accumulator receives its MFMAs in one fixed order (G ascending, four k-steps each).
// Pipeline: the reads and the transform of step s + 1 sit between the MFMAs of step s, V in two register sets that swap by name; U lives in two sets as well and
// rolls TWO steps ahead (a row of 2 positions has as few as 8 MFMAs): the set of step s takes the fragments of step s + 2 as its positions retire.  Both sets enter
// holding steps 0 and 1 (poly_prefetch_u, requested in front of the barrier before the layer).
constexpr int poly_row_np(int r) { return (r < 3 || (r >= 6 && r < 8)) ? 3 : 2; }
constexpr int poly_row_xi0(int r) { return r < 3 ? 3 * r : (r < 6 ? 9 + 2 * (r - 3) : (r < 8 ? 15 + 3 * (r - 6) : 21 + 2 * (r - 8))); }
constexpr bool poly_row_oddy(int r) { return r < 6; }
constexpr int poly_row_yi(int r) { return r < 3 ? r : (r < 6 ? r - 3 : (r < 8 ? r - 6 : r - 8)); }
constexpr int poly_row_ra(int r) { return poly_row_oddy(r) ? (poly_row_yi(r) == 0 ? 0 : 2) : 1 + 2 * poly_row_yi(r); }      // window row read into da
constexpr int poly_row_rb(int r) { return (poly_row_oddy(r) && poly_row_yi(r) != 1) ? (poly_row_yi(r) == 0 ? 2 : 4) : -1; }   // the row subtracted from it, or none
constexpr int poly_row_reads(int r) { return poly_row_np(r) * (poly_row_rb(r) >= 0 ? 2 : 1); }
constexpr int poly_row_valu(int r) { return 4 * ((poly_row_rb(r) >= 0 ? poly_row_np(r) : 0) + (poly_row_np(r) == 3 ? 2 : 0)); }

template <int... I, typename F>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, F&& f) { (f(IntC<I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) { static_for_seq(std::make_integer_sequence<int, N>{}, f); }

// The window rows of position row R at LDS byte address `ab` of the 5x5 window: columns 0, 2, 4 (odd phase) or 1, 3 (even phase)
template <typename LI, int R>
__device__ __forceinline__ void poly_read_row(unsigned ab, f32x4 (&da)[3], f32x4 (&db)[3]) {
    constexpr int NC = poly_row_np(R), C0 = NC == 3 ? 0 : 1, RA = poly_row_ra(R), RB = poly_row_rb(R);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        da[c] = lds_read4(ab + (RA * LI::WP + C0 + 2 * c) * 16);
        if constexpr (RB >= 0) db[c] = lds_read4(ab + (RB * LI::WP + C0 + 2 * c) * 16);
    }
}

// The V fragments of position row R from its window rows: along y (a difference of two rows or one row as it is), then along x
template <int R>
__device__ __forceinline__ void poly_transform_row(const f32x4 (&da)[3], const f32x4 (&db)[3], f32x4 (&V)[3]) {
    constexpr int NC = poly_row_np(R), RB = poly_row_rb(R);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t[3];
#pragma unroll
        for (int c = 0; c < NC; ++c) t[c] = RB >= 0 ? wsub(da[c][e], db[c][e]) : da[c][e];
        if constexpr (NC == 3) { V[0][e] = wsub(t[0], t[1]); V[1][e] = t[1]; V[2][e] = wsub(t[1], t[2]); }
        else { V[0][e] = t[0]; V[1][e] = t[1]; }
    }
}

// U of steps 0 and 1 of the wave's first unit
template <int NW, int CIN, int COUT, int HOUT, int NB, int NCB>
__device__ __forceinline__ void poly_prefetch_u(const float* __restrict__ Wu, f32x4 (&Ua)[NCB][3], f32x4 (&Ub)[NCB][3], int wave, int lane) {
    constexpr int NGRP = CIN / 16;
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(Wu, POLY_XI * CIN * COUT);
    const int u_lane = wino_u_lane<HOUT, COUT, NB>(wave, 0, lane);
    constexpr int R1 = 1 / NGRP, G1 = 1 % NGRP;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
            Ua[c][k] = wino_load_u<CIN, COUT>(r, u_lane, k, 0, c);
            if (k < poly_row_np(R1)) Ub[c][k] = wino_load_u<CIN, COUT>(r, u_lane, poly_row_xi0(R1) + k, G1, c);
        }
}

// Pre-activation outputs (no bias) of the NB passes in wino_tile's numbering over the OUTPUT (H = LI::H / 2): y[q][2 dy + dx] = couts 16 cb + 4 (lane >> 4) + 0..3
// of pixel (2 ty + dy, 2 tx + dx) - what wino_bias / wino_store_lds take.
template <int NW, int CIN, int COUT, typename LI, int NB, int NCB>
__device__ __forceinline__ void conv3x3_poly_mfma_rows(const float* act, const float* __restrict__ Wu, f32x4 (&Ua)[NCB][3], f32x4 (&Ub)[NCB][3], f32x4 (&y)[NB][4],
                                                       int wave, int lane) {
    constexpr int HOUT = LI::H / 2, HT = HOUT / 2, NGRP = CIN / 16, NSTEP = (NB / NCB) * 10 * NGRP;
    static_assert(LI::H % 4 == 0 && (HT * HT) % 16 == 0 && COUT % 16 == 0 && CIN % 16 == 0, "polyphase tiling");
    static_assert((HT * HT / 16) * (COUT / 16) == NW * NB, "the waves' passes must tile the layer exactly");
    static_assert((NCB == 1 || NCB == 2) && NB % NCB == 0 && (COUT / 16) % NCB == 0 && NSTEP % 2 == 0, "the passes of a unit must share their tile block");
    const int m = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wu, POLY_XI * CIN * COUT);
    f32x4 t0[NCB][5], t1[NCB][5], acc[NCB][3], Va[3], Vb[3];      // t0 / t1: the y stage, columns 0 .. 2 odd phase, 3 .. 4 even phase
    auto window_addr = [&](int u, int G) {
        int ty, tx, cb;
        wino_tile<HOUT, COUT, NB>(wave, NCB * u, m, ty, tx, cb);
        unsigned ab = lds_byte_addr(act) + (((4 * G + kq) * LI::PSG + (4 * ty * LI::WP + 4 * tx) * 4) * 4);
        asm("" : "+v"(ab));
        return ab;
    };
    // one step: the MFMAs of step S on V, with the reads + transform of step S + 1 (into Vn) and the U requests of step S + 2 (into this step's set) between them
    auto step = [&](auto sc, const f32x4 (&V)[3], f32x4 (&Vn)[3], f32x4 (&U)[NCB][3]) {
        constexpr int S = decltype(sc)::v;
        constexpr int u = S / (10 * NGRP), R = (S / NGRP) % 10, G = S % NGRP;
        constexpr bool more = S + 1 < NSTEP;
        constexpr int Sn = more ? S + 1 : S, un = Sn / (10 * NGRP), Rn = (Sn / NGRP) % 10, Gn = Sn % NGRP;
        constexpr int S2 = S + 2 < NSTEP ? S + 2 : S, u2 = S2 / (10 * NGRP), R2 = (S2 / NGRP) % 10, G2 = S2 % NGRP;   // (the last two steps re-request their own weights: unused)
        constexpr int NP = poly_row_np(R), NP2 = poly_row_np(R2), XI2 = poly_row_xi0(R2);
        constexpr int NM = NP * 4 * NCB, NRn = more ? poly_row_reads(Rn) : 0, VPM = NCB == 2 ? 2 : 4, NVM = more ? (poly_row_valu(Rn) + VPM - 1) / VPM : 0;
        static_assert(NM >= NRn + NVM, "the next step's reads and transform fit between this step's MFMAs");
        const int u_next = wino_u_lane<HOUT, COUT, NB>(wave, NCB * u2, lane);
        unsigned abn = 0;
        if constexpr (more) abn = window_addr(un, Gn);
        if constexpr (G == 0) {
#pragma unroll
            for (int c = 0; c < NCB; ++c)
#pragma unroll
                for (int k = 0; k < NP; ++k) acc[c][k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x4 da[3], db[3];
        if constexpr (more) poly_read_row<LI, Rn>(abn, da, db);
        if constexpr (NCB == 2) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {              // the two channel blocks' chains of position k interleave
                    acc[0][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[0][k][s4], V[k][s4], acc[0][k], 0, 0, 0);   // U^T x V
                    acc[1][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[1][k][s4], V[k][s4], acc[1][k], 0, 0, 0);
                }
#pragma unroll
                for (int k2 = k; k2 < (k == NP - 1 ? 3 : k + 1); ++k2)
                    if (k2 < NP2) {
                        U[0][k2] = wino_load_u<CIN, COUT>(wrsrc, u_next, XI2 + k2, G2, 0);
                        U[1][k2] = wino_load_u<CIN, COUT>(wrsrc, u_next, XI2 + k2, G2, 1);
                    }
            }
        } else {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)                    // the positions' chains interleave
#pragma unroll
                for (int k = 0; k < NP; ++k) acc[0][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[0][k][s4], V[k][s4], acc[0][k], 0, 0, 0);
#pragma unroll
            for (int k2 = 0; k2 < NP2; ++k2) U[0][k2] = wino_load_u<CIN, COUT>(wrsrc, u_next, XI2 + k2, G2, 0);
        }
        if constexpr (more) poly_transform_row<Rn>(da, db, Vn);
        // pinned order: the first MFMAs each followed by one row read, the last NVM MFMAs each by VPM operations of the transform (the reads have had the MFMAs
        // in between to return), the U requests where their registers retire
#pragma unroll
        for (int mi = 0; mi < NM; ++mi) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (mi < NRn) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (mi >= NM - NVM) __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);
            if (NCB == 2 && (mi + 1) % 8 == 0) {
                const int k = mi / 8;
                if (k < NP2) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
                if (k == NP - 1 && NP2 > NP) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
            }
            if (NCB == 1 && mi == NM - 1) __builtin_amdgcn_sched_group_barrier(0x020, NP2 == 3 ? 3 : 2, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (G == NGRP - 1) {                         // the row's sums over K are complete: y stage, rows first
            constexpr int C0 = NP == 3 ? 0 : 3, yi = poly_row_yi(R);
#pragma unroll
            for (int c = 0; c < NCB; ++c) {
#pragma unroll
                for (int j = 0; j < NP; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (poly_row_oddy(R)) {
                            if (yi == 0) t0[c][C0 + j][e] = acc[c][j][e];
                            else if (yi == 1) { t0[c][C0 + j][e] = wadd(t0[c][C0 + j][e], acc[c][j][e]); t1[c][C0 + j][e] = acc[c][j][e]; }
                            else t1[c][C0 + j][e] = wsub(t1[c][C0 + j][e], acc[c][j][e]);
                        } else {
                            if (yi == 0) t0[c][C0 + j][e] = wadd(t0[c][C0 + j][e], acc[c][j][e]);
                            else t1[c][C0 + j][e] = wadd(t1[c][C0 + j][e], acc[c][j][e]);
                        }
                    }
                if constexpr (R == 9) {                        // ... then columns
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        y[NCB * u + c][0][e] = wadd(wadd(t0[c][0][e], t0[c][1][e]), t0[c][3][e]);
                        y[NCB * u + c][1][e] = wadd(wsub(t0[c][1][e], t0[c][2][e]), t0[c][4][e]);
                        y[NCB * u + c][2][e] = wadd(wadd(t1[c][0][e], t1[c][1][e]), t1[c][3][e]);
                        y[NCB * u + c][3][e] = wadd(wsub(t1[c][1][e], t1[c][2][e]), t1[c][4][e]);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    {
        f32x4 da[3], db[3];
        poly_read_row<LI, 0>(window_addr(0, 0), da, db);
        poly_transform_row<0>(da, db, Va);
    }
    static_for<NSTEP / 2>([&](auto hc) {
        constexpr int S = 2 * decltype(hc)::v;
        step(IntC<S>{}, Va, Vb, Ua);
        step(IntC<S + 1>{}, Vb, Va, Ub);
    });
}

// ---- the same polyphase form for the 16-channel trunks (AffNet shape form 2, exact OriNet: conv2 16 -> 32 @16x16, conv4 32 -> 64 @8x8) -------------------------
// These kernels live on 128 registers per lane (two workgroups per CU), so the loop follows conv3x3_wino_mfma_rows' discipline and not conv3x3_poly_mfma_rows': ONE U
// V register set and small U sets, a step = one position row (3 or 2 positions) of ONE K group: the row's 2 .. 6 ds_read_b128 (requested under the row before), 0 .. 20
// VALU operations, then 3 or 2 x 4 MFMAs (the positions' chains interleave) and the row's fold into the y stage (t0 / t1, five columns each:
// poly_row_*, poly_read_row and poly_transform_row above, the fold and its order as in conv3x3_poly_mfma_rows).  Both layers give every wave exactly ten steps = 100 MFMAs
// (the direct form: 144):
//   conv2: 64 output tiles = 4 tile blocks x 2 channel blocks = one (tile block, channel block) unit per wave (wino_tile's numbering, NB = 1), CIN = 16 = one K group;
//   conv4: one tile block x 4 channel blocks x 2 K groups: wave 2 p + h runs channel block p on K group h and folds its own partial rows into a PARTIAL y; the pair adds
//          the two partial y in the fixed order K group 0 + K group 1 through LDS (poly16_combine), each wave finishing one output row of its tiles.
// U lives in TWO sets of three fragments and rolls two rows ahead, as in conv3x3_poly_mfma_rows and for its reason: a row has 8 or 12 MFMAs, 256 .. 384 cycles of
// the pipe, less than an L2 load takes - with one set one row ahead the ten steps ran at the load's latency (measured: conv2 9.2 k ticks against the direct form's 10.1 k).
// Both sets enter holding rows 0 and 1 (poly16_prefetch_u, requested in front of the barrier before the layer).  Wu = the layer's 25 positions, [xi][CIN/16][kq][COUT][4], derived on
// the device from the blob's taps (derive_u.hip: derive_u_kernel; poly_weight_transform).  tools/winograd_numerics.py: poly16_conv2 / poly16_conv4 mirror the order.
template <int CIN, int COUT>
__device__ __forceinline__ int poly16_u_lane(int cb, int G, int lane) {
    return ((lane >> 4) * COUT + cb * 16 + (lane & 15)) * 16 + G * (16 * COUT * 4);
}
template <int CIN, int COUT>
__device__ __forceinline__ void poly16_prefetch_u(const float* __restrict__ Wu, f32x4 (&Ua)[3], f32x4 (&Ub)[3], int cb, int G, int lane) {
    const __amdgpu_buffer_rsrc_t r = weight_rsrc(Wu, POLY_XI * CIN * COUT);
    const int u_lane = poly16_u_lane<CIN, COUT>(cb, G, lane);
    static_assert(poly_row_np(0) == 3 && poly_row_np(1) == 3, "rows 0 and 1 fill both sets");
#pragma unroll
    for (int k = 0; k < 3; ++k) Ua[k] = wino_load_u<CIN, COUT>(r, u_lane, k, 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) Ub[k] = wino_load_u<CIN, COUT>(r, u_lane, poly_row_xi0(1) + k, 0);
}

// Pre-activation outputs (no bias) of tile (ty, tx) of lane m = lane & 15 over K group G of the input: y[2 dy + dx] = couts 16 cb + 4 (lane >> 4) + 0..3 of pixel
// (2 ty + dy, 2 tx + dx).  cb and G are uniform over the wave.
template <int CIN, int COUT, typename LI>
__device__ __forceinline__ void conv3x3_poly16_mfma_rows(const float* act, const float* __restrict__ Wu, f32x4 (&Ua)[3], f32x4 (&Ub)[3], f32x4 (&y)[4], int ty, int tx, int cb, int G,
                                                         int lane) {
    static_assert(LI::H % 4 == 0 && COUT % 16 == 0 && CIN % 16 == 0, "polyphase tiling");
    const int kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(Wu, POLY_XI * CIN * COUT);
    const int u_lane = poly16_u_lane<CIN, COUT>(cb, G, lane);
    unsigned ab = lds_byte_addr(act) + (((4 * G + kq) * LI::PSG + (4 * ty * LI::WP + 4 * tx) * 4) * 4);
    asm("" : "+v"(ab));
    f32x4 t0[5], t1[5], acc[3], da[3], db[3], V[3];       // t0 / t1: the y stage, columns 0 .. 2 odd phase, 3 .. 4 even phase
    poly_read_row<LI, 0>(ab, da, db);
    poly_transform_row<0>(da, db, V);
    // one step: the reads of row R + 1, the MFMAs of row R on V and the set U, the requests of row R + 2 into that set, the fold of row R, the transform of row R + 1 into V
    auto step = [&](auto rc, f32x4 (&U)[3]) {
        constexpr int R = decltype(rc)::v, R2 = R + 2 < 10 ? R + 2 : R;
        constexpr int NP = poly_row_np(R), NP2 = R + 2 < 10 ? poly_row_np(R2) : 0, XI2 = poly_row_xi0(R2);
#pragma unroll
        for (int k = 0; k < NP; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_sched_barrier(0);                // pinned: the positions' chains interleave, the U requests and the next row's reads follow
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int k = 0; k < NP; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[k][s4], V[k][s4], acc[k], 0, 0, 0);   // U^T x V
#pragma unroll
        for (int k = 0; k < NP2; ++k) U[k] = wino_load_u<CIN, COUT>(wrsrc, u_lane, XI2 + k, 0);
        if constexpr (R < 9) poly_read_row<LI, (R < 9 ? R + 1 : R)>(ab, da, db);      // in flight under the fold
        __builtin_amdgcn_sched_barrier(0);
        constexpr int C0 = NP == 3 ? 0 : 3, yi = poly_row_yi(R);        // the row's sums over the wave's K group are complete: y stage, rows first
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (poly_row_oddy(R)) {
                    if (yi == 0) t0[C0 + j][e] = acc[j][e];
                    else if (yi == 1) { t0[C0 + j][e] = wadd(t0[C0 + j][e], acc[j][e]); t1[C0 + j][e] = acc[j][e]; }
                    else t1[C0 + j][e] = wsub(t1[C0 + j][e], acc[j][e]);
                } else {
                    if (yi == 0) t0[C0 + j][e] = wadd(t0[C0 + j][e], acc[j][e]);
                    else t1[C0 + j][e] = wadd(t1[C0 + j][e], acc[j][e]);
                }
            }
        if constexpr (R == 9) {                           // ... then columns
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[0][e] = wadd(wadd(t0[0][e], t0[1][e]), t0[3][e]);
                y[1][e] = wadd(wsub(t0[1][e], t0[2][e]), t0[4][e]);
                y[2][e] = wadd(wadd(t1[0][e], t1[1][e]), t1[3][e]);
                y[3][e] = wadd(wsub(t1[1][e], t1[2][e]), t1[4][e]);
            }
        }
        if constexpr (R < 9) poly_transform_row<(R < 9 ? R + 1 : R)>(da, db, V);
    };
    static_for<5>([&](auto hc) {
        constexpr int R = 2 * decltype(hc)::v;
        step(IntC<R>{}, Ua);
        step(IntC<R + 1>{}, Ub);
    });
}

// conv4's pair sum.  Wave 2 p + h holds the partial y of K group h; wave 2 p keeps output row dy = 0 of its tiles and hands y[2], y[3] over, wave 2 p + 1 keeps dy = 1 and
// hands y[0], y[1] over: 2 KB per wave at Poly16::X, behind conv3's output, which other waves still read when a wave writes its slot.  After the barrier every wave forms
// yo[dx] = (K group 0) + (K group 1) of its row: fixed for every patch and launch, no atomics.  conv4's output (16 plane groups of LayC4) ends in front of X, so the stores
// that follow need no second barrier against the partner's slot reads.  `lds` = the start of the activation buffer.
struct Poly16 {                                           // float offsets from the start of the activation buffer
    static constexpr int X = 8 * LayC3::PSG, X_FLOATS = 8 * 2 * 256;
};
__device__ __forceinline__ void poly16_combine(float* lds, const f32x4 (&y)[4], f32x4 (&yo)[2], int wave, int lane) {
    const int h = wave & 1;
    float* xw = lds + Poly16::X + (wave * 2 * 64 + lane) * 4;
    const float* xr = lds + Poly16::X + ((wave ^ 1) * 2 * 64 + lane) * 4;
#pragma unroll
    for (int k = 0; k < 2; ++k) *reinterpret_cast<f32x4*>(&xw[k * 256]) = h == 0 ? y[2 + k] : y[k];
    __syncthreads();                                      // the partner's half is in place; every wave has finished reading conv3's output
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const f32x4 o = *reinterpret_cast<const f32x4*>(&xr[k * 256]);
#pragma unroll
        for (int e = 0; e < 4; ++e) yo[k][e] = h == 0 ? wadd(y[k][e], o[e]) : wadd(o[e], y[2 + k][e]);
    }
}
