// Loop probes of the trunk layers (include/affnet_hip_probes.h, libaffnet_hip_probes.so only): the MFMA loop of one layer in isolation on the trunk's
// LDS footprint.  Not part of the product path.
#include "cnn_trunk.h"

#include "../../include/affnet_hip_probes.h"

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
