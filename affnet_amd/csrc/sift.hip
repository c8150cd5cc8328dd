// The reference's SIFT descriptor for gfx950: SIFTNet(patch_size=32) (pytorch_sift.py:30-94, 8 angular x
// 4 x 4 spatial bins), the descriptor the reference's own test() functions construct (train_AffNet_test_on_graffity.py:122).
//
// One wavefront per patch.  The 1024 pixels are loaded, or sampled from the pyramid with the PS = 32 base grid, into LDS; every
// elementwise step follows the reference's fp32 operation order (-ffp-contract=off): centred differences with replicate padding,
// magnitude, atan2, Gaussian window, soft angular binning.  Per pixel the wave keeps (b0, (1 - w1) mag, w1 mag) in LDS; lane L then
// forms outputs L and L + 64 (index = bin * 16 + cy * 4 + cx: angular bins L / 16 and L / 16 + 4 of spatial cell L % 16) as the
// 11 x 11 stride-6 cross-correlation with the pooling table, selecting its two bins per pixel exactly as the reference's
// (b0 == i) w0 + (b1 == i) w1 does.  The 121 terms are added in row-major tap order by one lane: no atomics, a fixed summation
// order, no register array indexed at run time.  The two L2 normalisations use the wave butterfly of handcrafted.hip.
// Rows and columns 29..31 of a patch reach no cell (cell c covers pixels 6 c .. 6 c + 10) and are not evaluated.
// The 32 x 32 window (4 KB) is a device table; the pooling table and the base grid travel by value.
#include <math.h>

#include "common.h"

#define SIFT_PS 32
#define SIFT_N (SIFT_PS * SIFT_PS)
#define SIFT_KS 11            // get_bin_weight_kernel_size_and_stride(32, 4) = (11, 6)
#define SIFT_STRIDE 6
#define SIFT_USED 29          // pixels 0..28 per axis reach a cell
// Row stride of the per-pixel arrays: the 16 cells of a wave read (6 cy + ky) * 36 + 6 cx + kx at once; 6 * 36 cy mod 64 =
// 0, 24, 48, 8 and 6 cx = 0, 6, 12, 18 give 16 different banks (the four lanes of a cell read one address).
#define SIFT_WS 36

struct SiftTables {
    float pk[SIFT_KS * SIFT_KS];   // getPoolingKernel(11) (pytorch_sift.py:19-25) as float32
    float base[SIFT_PS];           // affine_grid base coordinates for PS = 32
};

__device__ __forceinline__ float sift_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// patches != NULL: (n_max, 32, 32) patches, grid (n_max, 1);  NULL: sampled from the pyramid along lafs / ids, grid (n_max, B),
// rows >= count[image] are zeroed like HardNet's descriptor rows (hardnet_finish_kernel).
__global__ __launch_bounds__(64) void sift32_kernel(const float* __restrict__ patches, PyrTable pt, const float* __restrict__ lafs,
                                                    const int32_t* __restrict__ ids, const int32_t* __restrict__ count, int n_max, SiftTables tb,
                                                    const float* __restrict__ window, float clipval, float* __restrict__ desc) {
    __shared__ float px[SIFT_N];
    __shared__ float w0s[SIFT_USED * SIFT_WS];
    __shared__ float w1s[SIFT_USED * SIFT_WS];
    __shared__ int b0s[SIFT_USED * SIFT_WS];
    const size_t bi = blockIdx.y;
    const int n = count ? min(count[bi], n_max) : n_max;
    const size_t pidx = bi * n_max + blockIdx.x;
    const int lane = threadIdx.x;
    float* d = desc + pidx * 128;
    if ((int)blockIdx.x >= n) { d[lane] = 0.0f; d[64 + lane] = 0.0f; return; }
    if (patches) {
        for (int p = lane; p < SIFT_N; p += 64) px[p] = patches[pidx * SIFT_N + p];
    } else {
        int o = ids[3 * pidx], l = ids[3 * pidx + 1];
        o = o < 0 ? 0 : (o >= pt.n_octaves ? pt.n_octaves - 1 : o);
        l = l < 0 ? 0 : (l >= pt.n_levels ? pt.n_levels - 1 : l);
        const float* img = pt.lvl[o][l] + bi * pt.img_stride;
        const int h = pt.h[o], w = pt.w[o];
        const float* L = lafs + 6 * pidx;
        const float m = (float)(h < w ? h : w);
        const float t00 = L[0] * m, t01 = L[1] * m, t02 = L[2] * (float)w;
        const float t10 = L[3] * m, t11 = L[4] * m, t12 = L[5] * (float)h;
        for (int p = lane; p < SIFT_N; p += 64) {
            const int r = p >> 5, c = p & 31;
            px[p] = aff_sample_bilinear(img, h, w, t00, t01, t02, t10, t11, t12, tb.base[c], tb.base[r]);
        }
    }
    __syncthreads();
    for (int p = lane; p < SIFT_USED * SIFT_PS; p += 64) {
        const int r = p >> 5, c = p & 31;
        if (c >= SIFT_USED) continue;
        const int cm = c > 0 ? c - 1 : 0, cp = c + 1;                                 // replicate padding (c, r <= 28: no clamp above)
        const int rm = r > 0 ? r - 1 : 0, rp = r + 1;
        const float gx = px[r * SIFT_PS + cp] - px[r * SIFT_PS + cm];                 // taps [-1, 0, 1]
        const float gy = px[rp * SIFT_PS + c] - px[rm * SIFT_PS + c];
        float mag = sqrtf((gx * gx + gy * gy) + 1e-10f);
        const float ori = atan2f(gy, gx + 1e-8f);
        mag = mag * window[p];
        const float o_big = ((ori + 6.28318548f) / 6.28318548f) * 8.0f;               // (ori + 2 pi) / (2 pi) * 8, fp32 scalars
        const float b0f = floorf(o_big);
        const float w1 = o_big - b0f;
        const int q = r * SIFT_WS + c;
        b0s[q] = (int)b0f & 7;                                                        // ori in [-pi, pi]: b0f in 4..12
        w0s[q] = (1.0f - w1) * mag;
        w1s[q] = w1 * mag;
    }
    __syncthreads();
    const int cell = lane & 15, ba = lane >> 4, bb = ba + 4;
    const int org = (SIFT_STRIDE * (cell >> 2)) * SIFT_WS + SIFT_STRIDE * (cell & 3);
    float a0 = 0.0f, a1 = 0.0f;
    for (int ky = 0; ky < SIFT_KS; ++ky) {
#pragma unroll
        for (int kx = 0; kx < SIFT_KS; ++kx) {
            const int q = org + ky * SIFT_WS + kx;
            const int b0 = b0s[q], b1 = (b0 + 1) & 7;
            const float u0 = w0s[q], u1 = w1s[q];
            const float va = (b0 == ba ? u0 : 0.0f) + (b1 == ba ? u1 : 0.0f);
            const float vb = (b0 == bb ? u0 : 0.0f) + (b1 == bb ? u1 : 0.0f);
            const float k = tb.pk[ky * SIFT_KS + kx];
            a0 = fmaf(k, va, a0);
            a1 = fmaf(k, vb, a1);
        }
    }
    // L2Norm, clamp(0, clipval), L2Norm (pytorch_sift.py:91-93)
    float nrm = sqrtf(fabsf(sift_wave_sum(a0 * a0 + a1 * a1)) + 1e-10f);
    a0 = a0 / nrm; a1 = a1 / nrm;
    a0 = fminf(fmaxf(a0, 0.0f), clipval); a1 = fminf(fmaxf(a1, 0.0f), clipval);
    nrm = sqrtf(fabsf(sift_wave_sum(a0 * a0 + a1 * a1)) + 1e-10f);
    d[lane] = a0 / nrm;
    d[64 + lane] = a1 / nrm;
}

// getPoolingKernel(11): outer product in double of (0.1 0.3 0.5 0.7 0.9 1 0.9 0.7 0.5 0.3 0.1), cast to float32
static void sift_pooling_table(float* pk) {
    const int half = SIFT_KS / 2;
    const double step = 1.0 / (double)half;
    double xc[SIFT_KS];
    for (int i = 0; i < half; ++i) xc[i] = xc[SIFT_KS - 1 - i] = step / 2.0 + (double)i * step;
    xc[half] = 1.0;
    for (int y = 0; y < SIFT_KS; ++y)
        for (int x = 0; x < SIFT_KS; ++x) pk[y * SIFT_KS + x] = (float)(xc[y] * xc[x]);
}

static int sift_launch(affnet_ctx* ctx, const float* patches, const float* lafs, const int32_t* ids, const int32_t* count, int n_max,
                       const float* window, float clipval, float* desc, hipStream_t st) {
    if (!window || !desc || n_max < 0 || (!patches && (!lafs || !ids))) return aff_fail(ctx, AFFNET_ERR_INVALID, "sift: null argument");
    if (!patches && !ctx->ws) return aff_fail(ctx, AFFNET_ERR_INVALID, "sift: sampling from the pyramid needs a bound workspace");
    if (n_max == 0) return AFFNET_OK;
    SiftTables tb;
    sift_pooling_table(tb.pk);
    aff_base_grid(SIFT_PS, tb.base);
    PyrTable pt;
    if (!patches) aff_fill_pyr_table(ctx, &pt); else memset(&pt, 0, sizeof(pt));
    hipLaunchKernelGGL(sift32_kernel, dim3(n_max, patches ? 1 : ctx->B), dim3(64), 0, st, patches, pt, lafs, ids, count, n_max, tb, window, clipval,
                       desc);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// CircularGaussKernel(kernlen=32) of pytorch_sift.py:31-44 under Python 3 (halfSize = 16.0), evaluated in double, cast to float32
extern "C" int affnet_sift_host_window(int patch_size, float* h_out) {
    if (patch_size != SIFT_PS || !h_out) return AFFNET_ERR_INVALID;
    const double half = (double)patch_size / 2.0, r2 = half * half, sigma2 = 0.9 * r2;
    for (int y = 0; y < patch_size; ++y)
        for (int x = 0; x < patch_size; ++x) {
            const double disq = ((double)y - half) * ((double)y - half) + ((double)x - half) * ((double)x - half);
            h_out[y * patch_size + x] = disq < r2 ? (float)exp(-disq / sigma2) : 0.0f;
        }
    return AFFNET_OK;
}

extern "C" int affnet_sift_forward(affnet_ctx* ctx, const float* d_patches, int n, const float* d_window, float clipval, float* d_desc,
                                   void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_patches) return aff_fail(ctx, AFFNET_ERR_INVALID, "sift_forward: null argument");
    return sift_launch(ctx, d_patches, nullptr, nullptr, nullptr, n, d_window, clipval, d_desc, (hipStream_t)stream);
}

extern "C" int affnet_sift_forward_pyr(affnet_ctx* ctx, const float* d_lafs_norm, const int32_t* d_ids, const int32_t* d_count, int n_max,
                                       const float* d_window, float clipval, float* d_desc, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx) return AFFNET_ERR_INVALID;
    return sift_launch(ctx, nullptr, d_lafs_norm, d_ids, d_count, n_max, d_window, clipval, d_desc, (hipStream_t)stream);
}
