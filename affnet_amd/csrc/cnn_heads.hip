// What runs behind the trunk kernels of the 32x32-patch CNNs (cnn_trunk.h): the AffNet / OriNet finish kernels, HardNet's head GEMM and finish
// kernel, their launchers (called by cnn_launch, cnn32.hip), and the MFMA layout self-test.
#include <stdlib.h>

#include "common.h"

#include "cnn_mfma.h"
#include "shape_filter.h"

// ---- AffNet / OriNet heads, second half: combine the eight per-wave partials of a patch ---------------------------------
//   AffNet : + bias -> tanh -> [[1+x0, 0],[x1, 1+x2]] -> rectifyAffineTransformationUpIsUp
//            (architectures.py:227-229,246-252, LAF.py:285-291); one thread per patch; optionally the shape filter of the row
//            (laf_ops.hip: aff_shape_filter_row) in the same kernel - the fused pipeline's finish + filter
//   OriNet : + bias -> tanh -> mean over the 3x3 map -> atan2 -> rotation (architectures.py:56-58,76-82, LAF.py:276-283); one
//            WAVEFRONT per patch: lane q < 18 adds the eight partials of tap q (18 consecutive floats per wave partial: coalesced;
//            one thread per patch read 144 floats at a 576-byte stride, 5.8x overfetch, 18 us for 2000 patches), the nine tanh
//            values of each output are added in tap order as before; optionally LAF <- LAF * R in the same kernel
//            (SparseImgRepresenter.py:173-177).
// A of one row from its eight per-wave partials: shared by the finish kernel and the margin kernel, so that the margin rule sees the finish kernel's A
__device__ __forceinline__ f32x4 affnet_head_to_a(const float* __restrict__ part, const float* __restrict__ hb, size_t pidx) {
    const f32x4* pp = reinterpret_cast<const f32x4*>(part + pidx * HEAD_PART_AFF);
    f32x4 r[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) r[w] = pp[w];
    const f32x4 s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    const float x0 = tanhf(s.x + hb[0]), x1 = tanhf(s.y + hb[1]), x2 = tanhf(s.z + hb[2]);
    const float a00 = 1.0f + x0, a01 = 0.0f * x0, a10 = x1, a11 = 1.0f + x2;
    const float det = sqrtf(fabsf(a00 * a11 - a10 * a01 + 1e-10f));
    const float b2a2 = sqrtf(a01 * a01 + a00 * a00);
    return (f32x4){b2a2 / det, 0.0f * det, (a11 * a01 + a10 * a00) / (b2a2 * det), det / b2a2};
}

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
    const f32x4 A = affnet_head_to_a(part, hb, pidx);
    const float o0 = A.x, o1 = A.y, o2 = A.z, o3 = A.w;
    o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
    if (sf.key) {
        const size_t bi = blockIdx.y;
        aff_shape_filter_row(sf.resp + bi * n_max, sf.lafs + bi * n_max * 6, o0, o1, o2, o3, row, sf.key + bi * n_max, sf.good + bi * n_max,
                             sf.cnt + bi * CNT_TOTAL);
    }
}

// Shape form 1, between the Winograd AffNet trunk and the direct one: one thread per evaluated row of the window applies the margin rule (shape_filter.h) to
// the row's A and writes the row's flag; flagged rows are counted per image (CNT_AFF_REEVAL; cleared by the first pass's trunk launch).  The rows and the
// lazy predicate of the finish kernel; the trunk launch in front of this one has frozen CNT_SURVIVED1.
__global__ __launch_bounds__(256) void affnet_margin_kernel(const float* __restrict__ part, const float* __restrict__ hb, const int32_t* __restrict__ count,
                                                            int n_max, int row_begin, int row_end, const int32_t* __restrict__ skip_cnt, int skip_n,
                                                            const float* __restrict__ lafs, int32_t* __restrict__ flags, int32_t* __restrict__ cnt) {
    const int row = row_begin + blockIdx.x * 256 + threadIdx.x;
    const int n = min(count ? min(count[blockIdx.y], n_max) : n_max, row_end);
    if (row >= n || lazy_skip(skip_cnt, skip_n, blockIdx.y)) return;
    const size_t bi = blockIdx.y, pidx = bi * n_max + row;
    const f32x4 A = affnet_head_to_a(part, hb, pidx);
    const bool flag = aff_shape_margin_flag(lafs + bi * n_max * 6, A.x, A.y, A.z, A.w, row);
    flags[pidx] = flag ? 1 : 0;
    if (flag) atomicAdd(&cnt[bi * CNT_TOTAL + CNT_AFF_REEVAL], 1);
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

// AffNet / OriNet: combine the per-wave head partials in `scratch` (rows of the window)
int aff_finish_affnet(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int rows, int B) {
    ShapeFuse sf;
    memset(&sf, 0, sizeof(sf));
    if (c.fuse) sf = *c.fuse;
    hipLaunchKernelGGL(affnet_finish_kernel, dim3(aff_cdiv(rows, 256), B), dim3(256), 0, c.st, c.scratch, c.packed + L.head_b, c.count, c.n_max, c.out,
                       c.row_begin, c.row_begin + rows, c.skip_cnt, c.skip_n, sf);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

int aff_margin_affnet(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int rows, int B, int32_t* flags) {
    hipLaunchKernelGGL(affnet_margin_kernel, dim3(aff_cdiv(rows, 256), B), dim3(256), 0, c.st, c.scratch, c.packed + L.head_b, c.count, c.n_max, c.row_begin,
                       c.row_begin + rows, c.skip_cnt, c.skip_n, c.fuse->lafs, flags, c.fuse->cnt);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

int aff_finish_orinet(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int rows, int B) {
    DenormSel ds;
    memset(&ds, 0, sizeof(ds));
    if (c.denorm && c.rot_lafs) ds = *c.denorm;
    hipLaunchKernelGGL(orinet_finish_kernel, dim3(aff_cdiv(rows, 4), B), dim3(256), 0, c.st, c.scratch, c.packed + L.head_b, c.count, c.n_max, c.out,
                       c.row_begin, c.row_begin + rows, c.rot_lafs, ds);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// HardNet: head GEMM over all rows of the trunk output in `scratch` + finish kernel
int aff_hardnet_head(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int B) {
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
    const int ai = ctx->arith == AFFNET_ARITH_FP32_SPLIT2H ? 2 : (ctx->arith == AFFNET_ARITH_FP32_SPLIT3 ? 1 : 0);      // exact fp32, three bf16 terms, two fp16 terms
    const float* hw = c.packed + (ai == 2 ? L.head_h2 : (ai == 1 ? L.head_s3 : L.head_w));
    hipLaunchKernelGGL(heads[ai][mp == 64 ? 0 : (mp == 32 ? 1 : 2)], dim3(aff_cdiv(n_max, mp), HEAD_KSPLIT, B), dim3(256), 0, c.st, c.scratch, hw, c.count,
                       n_max, partial);
    AFF_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(hardnet_finish_kernel, dim3(aff_cdiv(n_max, 4), B), dim3(256), 0, c.st, partial, c.packed + L.head_b, c.count, n_max, c.out);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

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
