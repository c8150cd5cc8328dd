// conv5 of the exact HardNet trunk in descriptor form 3 (affnet_set_desc_form): 128 -> 128 channels at 8 x 8 as Winograd F(4x4, 3x3), FOUR consecutive patches per workgroup,
// behind the trunk of form 3 (cnn_trunk_hardnet_c5.hip), which leaves conv4's tensor in the patch's 32 KB slot.  One patch has four 4x4 tiles and the MFMA wants 16 columns; four
// patches give it a full block, and the layer costs 36 x 8 x 32 = 9216 MFMAs per four patches - 288 per wave and patch against the 512 of F(2x2, 3x3) inside the trunk.
// The layer's description, LDS layout and lane-local transforms: cnn_mfma.h (F43C5L, f43c5_transform, f43c5_output).  A unit of its own, as every kernel family here.
#include "cnn_mfma.h"

#define C5_STAMP(k)                                                                                                      \
    do {                                                                                                                 \
        if (STAMPS && a.dbg_time && lane == 0) a.dbg_time[(pidx0 * 8 + wave) * 32 + (k)] = __builtin_readcyclecounter(); \
    } while (0)

// grid = (groups of four rows, images), 8 waves.  The last group of an image's rows may hold 1 .. 3 real patches: the other columns of the M block are zero and are not stored.
// Same row window, row count and lazy predicate as the trunk launch in front of it, so a group's real rows are exactly the rows whose slots that launch wrote.
template <bool STAMPS>
__global__ __launch_bounds__(512, 2) void hardnet_conv5_f43_kernel(Conv5Args a) {
    constexpr int CIN = 128, COUT = 128, DU = 6, DV = 6;     // rolling register sets, U (L2) and V (LDS) 6 positions = 24 MFMAs ahead; 144 + 24 + 24 + 16 (next quarter's input) registers
    static_assert(F43_XI % DU == 0 && F43_XI % DV == 0 && DU % 2 == 0 && DV % 2 == 0, "the sets roll with compile-time indices");
    __shared__ __attribute__((aligned(16))) float lds[F43C5L::TOTAL];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = a.count ? min(a.count[blockIdx.y], a.n_max) : a.n_max;
    const int r0 = a.row_begin + 4 * blockIdx.x, rend = min(n, a.row_end);
    if (r0 >= rend || lazy_skip(a.skip_cnt, a.skip_n, blockIdx.y, CNT_SURVIVED)) return;
    const int nreal = min(4, rend - r0);
    const size_t pidx0 = (size_t)blockIdx.y * a.n_max + r0;
    float* slot = a.io + pidx0 * (64 * CIN);
    __builtin_amdgcn_s_setprio(3);
    C5_STAMP(24);

    // U of K group 0, positions 0 .. DU - 1: does not depend on the activations
    const __amdgpu_buffer_rsrc_t wrsrc = weight_rsrc(a.U, F43_XI * CIN * COUT);
    const int u_lane = ((lane >> 4) * COUT + wave * 16 + (lane & 15)) * 16;
    f32x4 Ur[DU], Vr[DV];
#pragma unroll
    for (int k = 0; k < DU; ++k) Ur[k] = wino_load_u<CIN, COUT>(wrsrc, u_lane, k, 0);

    // a quarter's input: patch i, channel group 8 Q + wave, pixel lane - 1 KB contiguous per wave and patch.  A column past the group's last real patch loads that
    // patch once more (no branch around a load) and becomes zero where it is stored to LDS
    f32x4 in[4];
    const float* src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) src[i] = slot + min(i, nreal - 1) * (64 * CIN) + (wave * 64 + lane) * 4;
    auto request = [&](int Q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) in[i] = *reinterpret_cast<const f32x4*>(src[i] + Q * (8 * 64 * 4));
    };
    request(0);
    // the halo of the 32 (patch, channel group) tiles: 36 cells each, written once (the quarters' interiors never touch it)
    for (int i = tid; i < 32 * 36; i += 512) {
        const int pc = i / 36, hp = i - pc * 36;
        const int y = hp < 10 ? 0 : (hp < 20 ? 9 : 1 + ((hp - 20) >> 1)), x = hp < 10 ? hp : (hp < 20 ? hp - 10 : ((hp - 20) & 1) * 9);
        *reinterpret_cast<f32x4*>(&lds[F43C5L::IN + (pc >> 3) * F43C5L::PS + (pc & 7) * F43C5L::CGS + (y * F43C5L::WPI + x) * 4]) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    float* in_w = &lds[F43C5L::IN + wave * F43C5L::CGS + (((lane >> 3) + 1) * F43C5L::WPI + (lane & 7) + 1) * 4];
    // the transform's thread: channel e of channel group `wave` of the quarter, window (patch tp, tile ty, tx); a 32-lane half = 4 channels x 2 tx x 4 patches: 32 banks
    const int te = lane & 3, ttx = (lane >> 2) & 1, tp = (lane >> 3) & 3, tty = lane >> 5;
    const float* t_in = &lds[F43C5L::IN + tp * F43C5L::PS + wave * F43C5L::CGS + (4 * tty * F43C5L::WPI + 4 * ttx) * 4 + te];
    float* t_v = &lds[F43C5L::V + (wave >> 2) * (F43_XI * 256) + ((wave & 3) * 16 + 4 * tp + 2 * tty + ttx) * 4 + te];
    const unsigned v0 = lds_byte_addr(lds + F43C5L::V) + lane * 16;

    f32x4 acc[F43_XI];
#pragma unroll
    for (int k = 0; k < F43_XI; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int Q = 0; Q < 4; ++Q) {
        // every wave is past the previous quarter's transform (which read IN) since the barrier in front of that quarter's loop
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(in_w + i * F43C5L::PS) = i < nreal ? in[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
        __syncthreads();                                  // the quarter's input is in place; every wave has finished the previous quarter's loop (V is free)
        if (Q == 0) C5_STAMP(25);
        // the next quarter: requested here so that it lands under the transform - vector memory loads retire in order, so the loop's first U fragments wait for it
        if (Q < 3) request(Q + 1);
        f43c5_transform(t_in, t_v);
        __syncthreads();                                  // V of the quarter is in place
        if (Q == 0) C5_STAMP(26);
        if (Q == 3) C5_STAMP(28);
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int k = 0; k < DV; ++k) Vr[k] = lds_read4(v0 + k * 1024);
#pragma unroll 1
        for (int Gq = 0; Gq < 2; ++Gq) {
            const int G = 2 * Q + Gq, Gn = G == CIN / 16 - 1 ? G : G + 1;     // (the last group re-requests itself: unused)
            unsigned vcur = v0 + Gq * (F43_XI * 1024), vnext = v0 + (1 - Gq) * (F43_XI * 1024);   // (the quarter's second group re-requests the first: unused)
            asm("" : "+v"(vcur));
            asm("" : "+v"(vnext));
            __builtin_amdgcn_sched_barrier(0);            // pinned: two positions' chains interleave, their U and V reloads follow
#pragma unroll
            for (int k = 0; k < F43_XI; k += 2) {
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ur[k % DU][s4], Vr[k % DV][s4], acc[k], 0, 0, 0);
                    acc[k + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ur[(k + 1) % DU][s4], Vr[(k + 1) % DV][s4], acc[k + 1], 0, 0, 0);
                }
#pragma unroll
                for (int kk = k; kk < k + 2; ++kk) {
                    const int ku = kk + DU, kv = kk + DV;
                    Ur[kk % DU] = ku < F43_XI ? wino_load_u<CIN, COUT>(wrsrc, u_lane, ku, G) : wino_load_u<CIN, COUT>(wrsrc, u_lane, ku - F43_XI, Gn);
                    Vr[kk % DV] = kv < F43_XI ? lds_read4(vcur + kv * 1024) : lds_read4(vnext + (kv - F43_XI) * 1024);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_s_setprio(3);
        if (Q == 0) C5_STAMP(27);
        if (Q == 3) C5_STAMP(29);
    }

    // The rewrite is IN PLACE: the group's four slots hold conv4's tensor until here and conv5's from here on.  Invariant: every wave of this workgroup has read all four
    // quarters of all four slots before the first store - the last quarter's loads were consumed (stored to LDS) in front of that quarter's first barrier; this barrier
    // enforces it for the whole workgroup.  No other workgroup touches these slots.
    __syncthreads();
    f32x4 y[16];
    f43c5_output(acc, y);
    const f32x4 bias = *reinterpret_cast<const f32x4*>(&a.bias[wave * 16 + 4 * (lane >> 4)]);
    C5_STAMP(30);
    const int m = lane & 15, op = m >> 2, oy = 4 * ((m >> 1) & 1), ox = 4 * (m & 1);
    if (op < nreal) {
        float* dst = slot + op * (64 * COUT) + wave * 16 + 4 * (lane >> 4);          // [pixel][channel]: wino_store_global's layout
#pragma unroll
        for (int k = 0; k < 16; ++k) *reinterpret_cast<f32x4*>(dst + ((oy + (k >> 2)) * 8 + ox + (k & 3)) * COUT) = bias_relu(y[k], bias);
    }
    C5_STAMP(31);
}

int aff_hardnet_conv5_f43(affnet_ctx* ctx, const Conv5Args& a, int groups, int B, bool stamps, hipStream_t st) {
    if (groups <= 0) return AFFNET_OK;
    hipLaunchKernelGGL(stamps ? hardnet_conv5_f43_kernel<true> : hardnet_conv5_f43_kernel<false>, dim3(groups, B), dim3(512), 0, st, a);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
