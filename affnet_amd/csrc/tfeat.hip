// The reference's HardTFeat descriptor for gfx950: HardTFeatNet.forward in eval mode (HardNet.py:30-59), the
// network the reference's test() functions build for --descriptor TFeat, with the trained weights of its HardTFeat.pth.
//
//   input norm (mean, unbiased std + 1e-7) -> conv 1 -> 32, 7 x 7 valid, tanh -> max-pool 2 x 2 -> conv 32 -> 64, 6 x 6 valid, tanh
//   -> conv 64 -> 128, 8 x 8 (a 4096 x 128 product), tanh -> x / sqrt(sum x^2 + 1e-8)
//
// Exact fp32 on v_mfma_f32_16x16x4_f32 throughout (12 605 696 FLOP per patch).  Three kernels:
//   * tfeat_trunk_kernel: one workgroup of four wavefronts per patch.  The patch is loaded, or sampled from the pyramid with the PS = 32
//     base grid exactly as affnet_pyr_grid_sample does, standardised and kept in LDS.
//     conv1 on the matrix cores with the PIXELS as the MFMA's rows: a tile is four pool windows x their four pixels (row 4 q + r = pixel r
//     of window q), K = 49 taps padded to 52 (the weight rows 49..51 are zero and the padded taps re-read the window's own pixel: finite),
//     N = 32 channels in two tiles.  A lane then holds the four pixels of ONE pool window of one channel: max, + bias, tanh in registers
//     (pool BEFORE tanh: a quarter of the tanhf calls; max(x) + b == max(x + b) exactly and tanh is monotone), no 26 x 26 tensor anywhere.
//     169 windows = 43 tiles, the last with one valid window (the others recompute window 168 and are dropped).  The pooled 13 x 13 x 32
//     tensor lives in LDS channel-interleaved by 4 (cnn_mfma.h), so one ds_read_b128 feeds four k-steps.
//     conv2 as an implicit GEMM like conv3x3_mfma: the WEIGHTS are the rows (wave w owns output channels 16 w .. 16 w + 15, its 72 KB of the
//     288 KB stream from L2 in w_tap_index order, one row of six taps ahead in registers), the 64 output pixels the columns in four tiles that
//     share every weight fragment; K = 36 taps x 32 channels.  + bias, tanh, and the 8 x 8 x 64 result goes to scratch as k = pixel * 64 +
//     channel (16-byte stores), the classifier GEMM's A order.
//   * tfeat_head_kernel: (n x 4096) x (4096 x 128) split-K GEMM after hardnet_head_kernel<64>: 64-patch tiles, four K quarters of 1024,
//     partial sums to scratch with plain stores.
//   * tfeat_finish_kernel: one wavefront per row adds the four partials in a fixed order, + bias, tanh, L2 norm; rows past the count = 0.
// Every sum has a fixed order that depends on nothing but the row's own data: a descriptor is the same bits whatever n, the batch, the
// row's position in a tile or the launch shape.  No atomics, no scratch memory.
#include <math.h>

#include "common.h"

#include "cnn_mfma.h"

#define TF_PS 32
#define TF_POOLW 13                  // pooled map 13 x 13
#define TF_NWIN (TF_POOLW * TF_POOLW)
#define TF_TILES1 ((TF_NWIN + 3) / 4)   // conv1 tiles of four pool windows: 43, the last with one valid window
#define TF_PSG 680                   // floats between the plane groups of the pooled tensor (169 pixels x 4 channels, padded)
#define TF_KSPLIT 4                  // K quarters of the classifier GEMM
#define TF_KC 128                    // K chunk per LDS slab of the classifier GEMM and its row stride
#define TF_AS (TF_KC + 4)
#define TF_MP 64                     // patches per workgroup of the classifier GEMM

struct TfBase { float base[TF_PS]; };   // affine_grid base coordinates for PS = 32

// patches != NULL: (n_max,32,32) patches, grid (n_max, 1);  NULL: sampled from the pyramid along lafs / ids, grid (n_max, B).
// Rows >= count[image] are left alone: the head GEMM reads them as zero and the finish kernel zeroes their descriptors.
__global__ __launch_bounds__(256) void tfeat_trunk_kernel(const float* __restrict__ packed, TfeatLayout L, const float* __restrict__ patches, PyrTable pt,
                                                          TfBase tb, const float* __restrict__ lafs, const int32_t* __restrict__ ids,
                                                          const int32_t* __restrict__ count, int n_max, float* __restrict__ trunk) {
    __shared__ float px[TF_PS * TF_PS];
    __shared__ __attribute__((aligned(16))) float act[8 * TF_PSG];
    __shared__ float red[8];
    const size_t bi = blockIdx.y;
    const int n = count ? min(count[bi], n_max) : n_max;
    if ((int)blockIdx.x >= n) return;
    const size_t pidx = bi * n_max + blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 15, kq = lane >> 4;

    // ---- patch + input norm (the HardNet trunk's: mean, unbiased std + 1e-7) --------------------------------------------------------
    float v[4];
    if (patches) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = patches[pidx * (TF_PS * TF_PS) + tid + 256 * q];
    } else {
        int o = ids[3 * pidx], l = ids[3 * pidx + 1];
        o = o < 0 ? 0 : (o >= pt.n_octaves ? pt.n_octaves - 1 : o);
        l = l < 0 ? 0 : (l >= pt.n_levels ? pt.n_levels - 1 : l);
        const float* img = pt.lvl[o][l] + bi * pt.img_stride;
        const int h = pt.h[o], w = pt.w[o];
        const float* F = lafs + 6 * pidx;
        const float mm = (float)(h < w ? h : w);
        const float t00 = F[0] * mm, t01 = F[1] * mm, t02 = F[2] * (float)w;
        const float t10 = F[3] * mm, t11 = F[4] * mm, t12 = F[5] * (float)h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = tid + 256 * q;
            v[q] = aff_sample_bilinear(img, h, w, t00, t01, t02, t10, t11, t12, tb.base[p & 31], tb.base[p >> 5]);
        }
    }
    const float mean = block_sum<4>((v[0] + v[1]) + (v[2] + v[3]), red) * (1.0f / 1024.0f);
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[q] -= mean; sq += v[q] * v[q]; }
    const float var = block_sum<4>(sq, red + 4) * (1.0f / 1023.0f);       // torch.std: unbiased
    const float sd = sqrtf(var) + 1e-7f;
#pragma unroll
    for (int q = 0; q < 4; ++q) px[tid + 256 * q] = v[q] / sd;

    // ---- conv1 + pool + bias + tanh ------------------------------------------------------------------------------------------------
    // this lane's share of the weights [k (52)][32] (the MFMA's B operand: k = 4 s + kq, channel 16 j + m) and of the tap offsets
    const float* w1 = packed + L.c1_w;
    float wb[TFEAT_K1 / 4][2];
    int toff[TFEAT_K1 / 4];
#pragma unroll
    for (int s = 0; s < TFEAT_K1 / 4; ++s) {
        const int k = 4 * s + kq;
        wb[s][0] = w1[k * 32 + m];
        wb[s][1] = w1[k * 32 + 16 + m];
        toff[s] = k < 49 ? (k / 7) * TF_PS + (k % 7) : 0;             // padded taps: zero weight x the window's own (finite) pixel
    }
    const float b1lo = packed[L.c1_b + m], b1hi = packed[L.c1_b + 16 + m];
    __syncthreads();
    for (int tile = wave; tile < TF_TILES1; tile += 4) {
        const int wnd = min(tile * 4 + (m >> 2), TF_NWIN - 1);             // row m of the tile: pixel m & 3 of this pool window
        const int wy = wnd / TF_POOLW, wx = wnd - wy * TF_POOLW;
        const float* a = px + (2 * wy + ((m >> 1) & 1)) * TF_PS + 2 * wx + (m & 1);     // + tap <= (25 + 6) * 32 + 25 + 6: inside the patch
        f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < TFEAT_K1 / 4; ++s) {
            const float av = a[toff[s]];
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wb[s][0], c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wb[s][1], c1, 0, 0, 0);
        }
        // c[r]: row 4 kq + r = pixel r of window 4 tile + kq, column m = channel (16 +) m
        const int ow = tile * 4 + kq;
        if (ow < TF_NWIN) {
            const float p0 = fmaxf(fmaxf(c0[0], c0[1]), fmaxf(c0[2], c0[3])), p1 = fmaxf(fmaxf(c1[0], c1[1]), fmaxf(c1[2], c1[3]));
            act[(m >> 2) * TF_PSG + ow * 4 + (m & 3)] = tanhf(p0 + b1lo);
            act[(4 + (m >> 2)) * TF_PSG + ow * 4 + (m & 3)] = tanhf(p1 + b1hi);
        }
    }
    __syncthreads();

    // ---- conv2 + bias + tanh -------------------------------------------------------------------------------------------------------
    // rows = output channels 16 wave + m (weights, lane (m, kq) = input channels 16 G + 4 kq + j), columns = pixels 16 t + m of tile t
    // (two output rows), K = (tap, G, kq, j)
    const __amdgpu_buffer_rsrc_t rw = weight_rsrc(packed + L.c2_w, 36 * 32 * 64);
    const int w_lane = (kq * 64 + wave * 16 + m) * 16;
    const unsigned b_addr = lds_byte_addr(act) + (kq * TF_PSG + ((m >> 3) * TF_POOLW + (m & 7)) * 4) * 4;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 wc[12], wn[12];
#pragma unroll
    for (int u = 0; u < 12; ++u) wc[u] = buf_read4(rw, w_lane, u * 4096);
#pragma unroll 1
    for (int ky = 0; ky < 6; ++ky) {
        if (ky + 1 < 6) {
#pragma unroll
            for (int u = 0; u < 12; ++u) wn[u] = buf_read4(rw, w_lane, ((ky + 1) * 12 + u) * 4096);
        }
        const unsigned row = b_addr + ky * (TF_POOLW * 16);
#pragma unroll
        for (int u = 0; u < 12; ++u) {                                  // u = kx * 2 + G
            f32x4 bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) bv[t] = lds_read4(row + (u & 1) * (4 * TF_PSG * 4) + (u >> 1) * 16 + t * (2 * TF_POOLW * 16));
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u][j], bv[t][j], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 12; ++u) wc[u] = wn[u];
    }
    // acc[t][r]: channel 16 wave + 4 kq + r of pixel 16 t + m
    const f32x4 b2 = *reinterpret_cast<const f32x4*>(packed + L.c2_b + wave * 16 + 4 * kq);
    float* o = trunk + pidx * TFEAT_HEAD_K + wave * 16 + 4 * kq;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f32x4 r;
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = tanhf(acc[t][q] + b2[q]);
        *reinterpret_cast<f32x4*>(o + (16 * t + m) * 64) = r;
    }
}

// The classifier as a split-K GEMM, after hardnet_head_kernel<64> (cnn_heads.hip): one workgroup = 64 patches x 128 outputs x one K quarter
// (1024); wave w owns outputs 32 w .. 32 w + 31 for the four 16-patch tiles.  The A slab (64 x 128) is fetched one iteration ahead through a
// buffer descriptor that ends behind the tile's last valid row (rows >= n read as zero).
__global__ __launch_bounds__(256, 2) void tfeat_head_kernel(const float* __restrict__ trunk, const float* __restrict__ Bw,
                                                            const int32_t* __restrict__ count, int n_max, float* __restrict__ partial) {
    constexpr int MI = TF_MP / 16, NA = TF_MP * TF_KC / 4 / 256, KQ = TFEAT_HEAD_K / TF_KSPLIT;
    __shared__ __attribute__((aligned(16))) float As[TF_MP * TF_AS];
    const int n = count ? min(count[blockIdx.z], n_max) : n_max;      // blockIdx.z = image of the batch
    const int p0 = blockIdx.x * TF_MP;
    if (p0 >= n) return;
    const size_t rows_total = (size_t)gridDim.z * n_max;
    const int kbeg = blockIdx.y * KQ;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t rA = weight_rsrc(trunk + ((size_t)blockIdx.z * n_max + p0) * TFEAT_HEAD_K, min(n - p0, TF_MP) * TFEAT_HEAD_K);
    const __amdgpu_buffer_rsrc_t rB = weight_rsrc(Bw, TFEAT_HEAD_K * 128);
    int offA[NA];
#pragma unroll
    for (int r = 0; r < NA; ++r) {
        const int f = tid + 256 * r, row = f >> 5, c4 = f & 31;       // 32 consecutive float4 = one 512-byte row segment
        offA[r] = (row * TFEAT_HEAD_K + 4 * c4) * 4;
    }
    const int offB = ((kq * 128) + wave * 32 + m) * 16;
    const unsigned a_addr = lds_byte_addr(As) + (m * TF_AS + 4 * kq) * 4;
    f32x4 acc[MI][2], stage[NA];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NA; ++r) stage[r] = buf_read4(rA, offA[r], kbeg * 4);
#pragma unroll 1
    for (int k0 = kbeg; k0 < kbeg + KQ; k0 += TF_KC) {
        __syncthreads();                                              // the previous slab has been consumed
#pragma unroll
        for (int r = 0; r < NA; ++r) {
            const int f = tid + 256 * r, row = f >> 5, c4 = f & 31;
            *reinterpret_cast<f32x4*>(&As[row * TF_AS + 4 * c4]) = stage[r];
        }
        __syncthreads();
        if (k0 + TF_KC < kbeg + KQ) {
#pragma unroll
            for (int r = 0; r < NA; ++r) stage[r] = buf_read4(rA, offA[r], (k0 + TF_KC) * 4);
        }
        f32x4 fa[2][MI], fb[2][2];
#pragma unroll
        for (int i = 0; i < MI; ++i) fa[0][i] = lds_read4(a_addr + i * 16 * TF_AS * 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[0][j] = buf_read4(rB, offB + j * 256, k0 * 512);
#pragma unroll
        for (int g = 0; g < TF_KC / 16; ++g) {
            const int cur = g & 1, nxt = cur ^ 1;
            if (g + 1 < TF_KC / 16) {
#pragma unroll
                for (int i = 0; i < MI; ++i) fa[nxt][i] = lds_read4(a_addr + i * 16 * TF_AS * 4 + (g + 1) * 64);
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
    // acc[i][j][r]: patch p0 + 16 i + 4 (lane>>4) + r, output 32 wave + 16 j + (lane & 15)
    float* dst = partial + ((size_t)blockIdx.y * rows_total + (size_t)blockIdx.z * n_max) * 128;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = p0 + 16 * i + 4 * kq + r;
            if (row >= n) continue;
            dst[(size_t)row * 128 + wave * 32 + m] = acc[i][0][r];
            dst[(size_t)row * 128 + wave * 32 + 16 + m] = acc[i][1][r];
        }
}

// One wavefront per row: the four K-quarter partials in fixed order, + bias, tanh, x / sqrt(sum x^2 + 1e-8) (L2Norm, HardNet.py:12-19).
// Rows past the image's row count are cleared here.
__global__ __launch_bounds__(256) void tfeat_finish_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                                           const int32_t* __restrict__ count, int n_max, float* __restrict__ out) {
    const int n = count ? min(count[blockIdx.y], n_max) : n_max;      // blockIdx.y = image of the batch
    const int lrow = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (lrow >= n_max) return;
    const size_t rows_total = (size_t)gridDim.y * n_max, row = (size_t)blockIdx.y * n_max + lrow;
    if (lrow >= n) { out[row * 128 + lane] = 0.0f; out[row * 128 + 64 + lane] = 0.0f; return; }
    float v0 = 0.f, v1 = 0.f;
#pragma unroll
    for (int s = 0; s < TF_KSPLIT; ++s) {
        const float* p = partial + ((size_t)s * rows_total + row) * 128;
        v0 += p[lane]; v1 += p[64 + lane];
    }
    v0 = tanhf(v0 + bias[lane]); v1 = tanhf(v1 + bias[64 + lane]);
    const float nrm = sqrtf(wave_sum(v0 * v0 + v1 * v1) + 1e-8f);
    out[row * 128 + lane] = v0 / nrm;
    out[row * 128 + 64 + lane] = v1 / nrm;
}

static int tfeat_launch(affnet_ctx* ctx, const float* packed, const float* patches, const float* lafs, const int32_t* ids, const int32_t* count,
                        int n_max, float* desc, float* scratch, hipStream_t st) {
    if (!packed || !desc || n_max < 0 || (!patches && (!lafs || !ids))) return aff_fail(ctx, AFFNET_ERR_INVALID, "tfeat: null argument");
    if (!patches && !ctx->ws) return aff_fail(ctx, AFFNET_ERR_INVALID, "tfeat: sampling from the pyramid needs a bound workspace");
    if (n_max == 0) return AFFNET_OK;
    if (!scratch) return aff_fail(ctx, AFFNET_ERR_INVALID, "tfeat: null scratch");
    const int B = patches ? 1 : ctx->B;
    const TfeatLayout L = tfeat_layout();
    TfBase tb;
    aff_base_grid(TF_PS, tb.base);
    PyrTable pt;
    if (!patches) aff_fill_pyr_table(ctx, &pt); else memset(&pt, 0, sizeof(pt));
    float* partial = scratch + (size_t)B * n_max * TFEAT_HEAD_K;      // [TF_KSPLIT][B * n_max][128] behind conv2's output
    hipLaunchKernelGGL(tfeat_trunk_kernel, dim3(n_max, B), dim3(256), 0, st, packed, L, patches, pt, tb, lafs, ids, count, n_max, scratch);
    AFF_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(tfeat_head_kernel, dim3(aff_cdiv(n_max, TF_MP), TF_KSPLIT, B), dim3(256), 0, st, scratch, packed + L.head_w, count, n_max, partial);
    AFF_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(tfeat_finish_kernel, dim3(aff_cdiv(n_max, 4), B), dim3(256), 0, st, partial, packed + L.head_b, count, n_max, desc);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

extern "C" size_t affnet_tfeat_scratch_floats(int rows) {
    return rows > 0 ? (size_t)rows * (TFEAT_HEAD_K + TF_KSPLIT * 128) : 0;
}

extern "C" int affnet_tfeat_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, const int32_t* d_count, int n_max,
                                    float* d_desc, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_patches) return aff_fail(ctx, AFFNET_ERR_INVALID, "tfeat_forward: null argument");
    return tfeat_launch(ctx, d_packed, d_patches, nullptr, nullptr, d_count, n_max, d_desc, d_scratch, (hipStream_t)stream);
}

extern "C" int affnet_tfeat_forward_pyr(affnet_ctx* ctx, const float* d_packed, const float* d_lafs_norm, const int32_t* d_ids,
                                        const int32_t* d_count, int n_max, float* d_desc, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx) return AFFNET_ERR_INVALID;
    return tfeat_launch(ctx, d_packed, nullptr, d_lafs_norm, d_ids, d_count, n_max, d_desc, d_scratch, (hipStream_t)stream);
}
