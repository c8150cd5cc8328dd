// Descriptor matching for gfx950 (the first consumer of the descriptors).
//
// Replaces Losses.py:5-13 (distance_matrix_vector), the second-nearest-neighbour ratio test of
// train_AffNet_test_on_graffity.py:292-300 and ReprojectionStuff.py:9-40,126-137 (linH, reprojectLAFs,
// get_GT_correspondence_indexes).
//
// The n1 x n2 distance matrix (36 MB at 3000 x 3000) is never materialised: rowmin_dist_kernel computes 64 x 16 tiles
// of a.b on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, K = descriptor length), turns them into
// sqrt((|a|^2 + |b|^2) - 2 a.b + 1e-6) in the reference's operation order and keeps a running (min, argmin) per row.
// The reference finds the "second nearest" by overwriting the COLUMNS of all nearest neighbours with 100000
// (dist_matrix[:, idxs_in_2] = 100000) and taking the row minimum again: the same kernel runs a second time with a
// per-column `used` mask, so the quirk (a column masked for every row, not only for its own) is reproduced.
// affnet_match_snn_many runs the same stages for P image pairs per launch (the pair index on a grid dimension, the segments from a device table).
#include <math.h>

#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The bodies below are the kernels of one image pair; every __global__ kernel of this file, single-pair or batched (pair index on a grid
// dimension, further down), only chooses the pointers and the workgroup index `blk` they run on.
__device__ __forceinline__ void sqnorm_body(const float* __restrict__ x, int n, int dim, float* __restrict__ out, int blk) {
    // one wavefront per row; torch.sum(a * a, dim=1)
    const int row = blk * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    float s = 0.f;
    for (int k = lane; k < dim; k += 64) { const float v = x[(size_t)row * dim + k]; s = fmaf(v, v, s); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[row] = s;
}

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ x, int n, int dim, float* __restrict__ out) {
    sqnorm_body(x, n, dim, out, blockIdx.x);
}

void aff_sqnorm_launch(hipStream_t st, const float* x, int n, int dim, float* out) {
    if (n > 0) hipLaunchKernelGGL(sqnorm_kernel, dim3(aff_cdiv(n, 4)), dim3(256), 0, st, x, n, dim, out);
}

// Workgroup = 4 wavefronts = 64 rows of `a`; wave w owns rows 16w..16w+15 and walks all columns of `b` in tiles of 16.
// MFMA roles: A operand = a rows (lane (m, kq) holds a[row m][16 t + 4 kq + j]), B operand = b rows (columns of the
// distance matrix); the K order is permuted identically on both sides, which a dot product does not see.
// Result tile: lane (n = l & 15, g = l >> 4) holds D[row 4 g + r][col n], r = 0..3.
//
// STAGE (the batched kernel): the four waves of a workgroup want the same 16 columns of `b`, so the workgroup loads each tile once (every thread
// DIM / 64 float4, the next tile's in flight during the MFMAs of this one), keeps it in one of two LDS buffers `s_b` (ROWMIN_BS floats per column:
// the 16-byte skew spreads the 16 columns over the banks) and every wave takes its B fragments from there.  The fragments hold the same values
// in the same lanes, so nothing after the load differs.  One barrier per tile, which every wave of the workgroup must reach: a wave whose 16 rows
// lie behind n1 computes on clamped rows like the tail lanes of a partial wave and writes nothing.
#define ROWMIN_BS(DIM) ((DIM) + 4)
template <int DIM, bool STAGE>
__device__ __forceinline__ void rowmin_dist_body(const float* __restrict__ a, int n1, const float* __restrict__ b, int n2,
                                                 const float* __restrict__ a_sq, const float* __restrict__ b_sq,
                                                 const uint8_t* __restrict__ used, float* __restrict__ out_min,
                                                 int32_t* __restrict__ out_idx, float* __restrict__ out_full, int blk, float* s_b) {
    constexpr int NG = DIM / 16;
    constexpr int BS = ROWMIN_BS(DIM), Q = DIM / 4, NPRE = 16 * Q / 256;      // float4 per column, float4 per thread and tile
    static_assert(!STAGE || (16 * Q) % 256 == 0, "the staged tile is loaded by 256 threads in whole rounds");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 15, kq = lane >> 4;
    const int row0 = blk * 64 + wave * 16;
    if (STAGE ? blk * 64 >= n1 : row0 >= n1) return;      // STAGE: uniform over the workgroup
    f32x4 fa[NG];
    {
        const int r = min(row0 + m, n1 - 1);
#pragma unroll
        for (int t = 0; t < NG; ++t) fa[t] = *reinterpret_cast<const f32x4*>(&a[(size_t)r * DIM + 16 * t + 4 * kq]);
    }
    float asq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) asq[r] = a_sq[min(row0 + 4 * kq + r, n1 - 1)];
    float best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    int bidx[4] = {0, 0, 0, 0};
    f32x4 pre[STAGE ? NPRE : 1];
    // tile at column c0 -> registers (columns clamped like the fragment loads of the direct form); registers -> LDS buffer `buf`
    auto tile_fetch = [&](int c0) {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int e = (int)threadIdx.x + 256 * j;
            pre[j] = *reinterpret_cast<const f32x4*>(&b[(size_t)min(c0 + e / Q, n2 - 1) * DIM + 4 * (e % Q)]);
        }
    };
    auto tile_store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int e = (int)threadIdx.x + 256 * j;
            *reinterpret_cast<f32x4*>(&s_b[buf * 16 * BS + (e / Q) * BS + 4 * (e % Q)]) = pre[j];
        }
    };
    if (STAGE) {
        tile_fetch(0);
        tile_store(0);
        __syncthreads();
    }
    for (int c0 = 0; c0 < n2; c0 += 16) {
        const int col = c0 + m;
        const int cc = min(col, n2 - 1);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        f32x4 fb[NG];
        const int buf = (c0 >> 4) & 1;
        const bool more = c0 + 16 < n2;
        float bsq = 0.f;
        bool masked = false;
        if (STAGE) {
            if (more) tile_fetch(c0 + 16);
            // in front of the MFMAs here: the two loads complete under them, and no branch (the null test of `used`) stands between the last
            // MFMA and the accumulator reads - with one there, a build of this form read acc[3] too early on the NULL path (NOTES.md)
            bsq = b_sq[cc];
            masked = used && used[cc];
#pragma unroll
            for (int t = 0; t < NG; ++t) fb[t] = *reinterpret_cast<const f32x4*>(&s_b[buf * 16 * BS + m * BS + 16 * t + 4 * kq]);
        } else {
#pragma unroll
            for (int t = 0; t < NG; ++t) fb[t] = *reinterpret_cast<const f32x4*>(&b[(size_t)cc * DIM + 16 * t + 4 * kq]);
        }
#pragma unroll
        for (int t = 0; t < NG; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t][j], fb[t][j], acc, 0, 0, 0);
        if (!STAGE) {
            bsq = b_sq[cc];
            masked = used && used[cc];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // Losses.py:12-13: sqrt((d1_sq + d2_sq) - 2.0 * a.b + eps)
            float d = sqrtf(((asq[r] + bsq) - 2.0f * acc[r]) + 1e-6f);
            if (masked) d = 100000.0f;
            // strict <: the first minimum wins; a NaN (the fp32 expansion can go below -1e-6 for near-identical vectors)
            // is sticky, as in torch.min
            if (col < n2 && (d < best[r] || (d != d && best[r] == best[r]))) { best[r] = d; bidx[r] = col; }
            if (out_full && col < n2 && row0 + 4 * kq + r < n1) out_full[(size_t)(row0 + 4 * kq + r) * n2 + col] = d;
        }
        if (STAGE) {        // the other buffer was last read one tile ago, in front of that tile's barrier
            if (more) tile_store(buf ^ 1);
            __syncthreads();
        }
    }
    // minimum over the 16 column lanes (same g): butterfly inside each row of 16 lanes, ties -> smaller column
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best[r], o, 64);
            const int oi = __shfl_xor(bidx[r], o, 64);
            const bool onan = ob != ob, bnan = best[r] != best[r];
            if ((onan && (!bnan || oi < bidx[r])) || (!onan && !bnan && (ob < best[r] || (ob == best[r] && oi < bidx[r])))) {
                best[r] = ob; bidx[r] = oi;
            }
        }
        const int row = row0 + 4 * kq + r;
        if (m == 0 && row < n1 && out_min) { out_min[row] = best[r]; out_idx[row] = bidx[r]; }
    }
}

template <int DIM>
__global__ __launch_bounds__(256) void rowmin_dist_kernel(const float* __restrict__ a, int n1, const float* __restrict__ b, int n2,
                                                          const float* __restrict__ a_sq, const float* __restrict__ b_sq,
                                                          const uint8_t* __restrict__ used, float* __restrict__ out_min,
                                                          int32_t* __restrict__ out_idx, float* __restrict__ out_full) {
    rowmin_dist_body<DIM, false>(a, n1, b, n2, a_sq, b_sq, used, out_min, out_idx, out_full, blockIdx.x, nullptr);
}

__device__ __forceinline__ void mark_used_body(const int32_t* __restrict__ idx, int n1, uint8_t* __restrict__ used, int blk) {
    const int i = blk * blockDim.x + threadIdx.x;
    if (i < n1) used[idx[i]] = 1;
}

__global__ void mark_used_kernel(const int32_t* __restrict__ idx, int n1, uint8_t* __restrict__ used) { mark_used_body(idx, n1, used, blockIdx.x); }

// One workgroup: ratio test + order-preserving compaction of the tentative matches (train_AffNet_test_on_graffity.py:296-300).
__device__ __forceinline__ void snn_select_body(const float* __restrict__ min1, const float* __restrict__ min2, const int32_t* __restrict__ idx, int n1,
                                                float thr, int32_t* __restrict__ tent, int32_t* __restrict__ count) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i0 = 0; i0 < n1; i0 += 1024) {
        const int i = i0 + threadIdx.x;
        bool keep = false;
        if (i < n1) keep = (min1[i] / (min2[i] + 1e-8f)) <= thr;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (keep) {
            const int slot = off + __popcll(bal & ((1ull << lane) - 1ull));
            tent[2 * slot] = i; tent[2 * slot + 1] = idx[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += s_wave[w]; s_base += t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = s_base;
}

__global__ __launch_bounds__(1024) void snn_select_kernel(const float* __restrict__ min1, const float* __restrict__ min2,
                                                          const int32_t* __restrict__ idx, int n1, float thr, int32_t* __restrict__ tent,
                                                          int32_t* __restrict__ count) {
    snn_select_body(min1, min2, idx, n1, thr, tent, count);
}

extern "C" int affnet_match_snn(affnet_ctx* ctx, const float* d_desc1, int n1, const float* d_desc2, int n2, int dim, float snn_threshold,
                                float* d_min_dist, int32_t* d_idx, float* d_min2_dist, int32_t* d_tent, int32_t* d_count, void* d_scratch,
                                void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_desc1 || !d_desc2 || !d_min_dist || !d_idx || !d_min2_dist || !d_tent || !d_count || !d_scratch || n1 < 0 || n2 < 1)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "match_snn: bad argument");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_snn: descriptor length %d (only 128 is built)", dim);
    hipStream_t st = (hipStream_t)stream;
    { int zrc = aff_zero_async(ctx, d_count, sizeof(int32_t), st); if (zrc) return zrc; }
    if (n1 == 0) return AFFNET_OK;
    float* a_sq = (float*)d_scratch;
    float* b_sq = a_sq + n1;
    uint8_t* used = (uint8_t*)(b_sq + n2);
    int32_t* idx2 = (int32_t*)(used + aff_align((size_t)n2, 16));
    { int zrc = aff_zero_async(ctx, used, (size_t)n2, st); if (zrc) return zrc; }
    aff_sqnorm_launch(st, d_desc1, n1, dim, a_sq);
    aff_sqnorm_launch(st, d_desc2, n2, dim, b_sq);
    hipLaunchKernelGGL(rowmin_dist_kernel<128>, dim3(aff_cdiv(n1, 64)), dim3(256), 0, st, d_desc1, n1, d_desc2, n2, a_sq, b_sq,
                       (const uint8_t*)nullptr, d_min_dist, d_idx, (float*)nullptr);
    hipLaunchKernelGGL(mark_used_kernel, dim3(aff_cdiv(n1, 256)), dim3(256), 0, st, d_idx, n1, used);
    hipLaunchKernelGGL(rowmin_dist_kernel<128>, dim3(aff_cdiv(n1, 64)), dim3(256), 0, st, d_desc1, n1, d_desc2, n2, a_sq, b_sq,
                       (const uint8_t*)used, d_min2_dist, idx2, (float*)nullptr);
    hipLaunchKernelGGL(snn_select_kernel, dim3(1), dim3(1024), 0, st, d_min_dist, d_min2_dist, d_idx, n1, snn_threshold, d_tent, d_count);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// Full distance matrix (Losses.py:5-13) for callers that want it: d_out (n1, n2).
extern "C" int affnet_distance_matrix(affnet_ctx* ctx, const float* d_desc1, int n1, const float* d_desc2, int n2, int dim, float* d_out,
                                      void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_desc1 || !d_desc2 || !d_out || !d_scratch || n1 < 0 || n2 < 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "distance_matrix: bad argument");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "distance_matrix: descriptor length %d (only 128 is built)", dim);
    if (n1 == 0 || n2 == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    float* a_sq = (float*)d_scratch;
    float* b_sq = a_sq + n1;
    aff_sqnorm_launch(st, d_desc1, n1, dim, a_sq);
    aff_sqnorm_launch(st, d_desc2, n2, dim, b_sq);
    hipLaunchKernelGGL(rowmin_dist_kernel<128>, dim3(aff_cdiv(n1, 64)), dim3(256), 0, st, d_desc1, n1, d_desc2, n2, a_sq, b_sq,
                       (const uint8_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, d_out);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

extern "C" size_t affnet_match_scratch_bytes(int n1, int n2) {
    return (size_t)(n1 + n2) * sizeof(float) + aff_align((size_t)n2, 16) + (size_t)n1 * sizeof(int32_t) + 64;
}

// ---- many pairs in one call: the pair index on a grid dimension of every stage -------------------------------------------------------------
// One pair fills an eighth of the part at best (cdiv(2000, 64) = 32 workgroups of the row-minimum kernel on 256 CUs, one workgroup for the
// selection); P independent pairs are P x that in the same six launches.  Every kernel reads its row of the pair table, tests it (aff_pair_row)
// and then runs the single-pair body above on the pair's segments, so a pair's outputs are the single-pair call's bit for bit.  Workgroups past
// the pair's own n1 leave through the body's own test, uniformly.
struct SnnMany {
    const float* desc1; int rows1;
    const float* desc2; int rows2;
    const int32_t* pairs;
    int n1_max, n2_max;
    float* a_sq; float* b_sq;          // scratch: (P, n1_max), (P, n2_max)
    uint8_t* used; int used_pitch;     // scratch: (P, used_pitch)
};

// false: the row is out of range, or the pair is empty - nothing to do either way (d_count was cleared)
__device__ __forceinline__ bool snn_many_row(const SnnMany& m, int p, AffPairRow& r) {
    return aff_pair_row(m.pairs, p, m.rows1, m.rows2, m.n1_max, m.n2_max, r) && r.n1 > 0 && r.n2 > 0;
}

// grid (rows / 4, P, side)
__global__ __launch_bounds__(256) void sqnorm_many_kernel(SnnMany m, int dim) {
    const int p = blockIdx.y;
    AffPairRow r;
    if (!snn_many_row(m, p, r)) return;
    if (blockIdx.z == 0) sqnorm_body(m.desc1 + (size_t)r.row1 * dim, r.n1, dim, m.a_sq + (size_t)p * m.n1_max, blockIdx.x);
    else sqnorm_body(m.desc2 + (size_t)r.row2 * dim, r.n2, dim, m.b_sq + (size_t)p * m.n2_max, blockIdx.x);
}

void aff_sqnorm_many_launch(hipStream_t st, const float* desc1, int rows1, const float* desc2, int rows2, int dim, const int32_t* pairs, int n_pairs,
                            int n1_max, int n2_max, float* a_sq, float* b_sq) {
    if (n_pairs <= 0 || n1_max <= 0 || n2_max <= 0) return;
    SnnMany m;
    m.desc1 = desc1; m.rows1 = rows1; m.desc2 = desc2; m.rows2 = rows2; m.pairs = pairs; m.n1_max = n1_max; m.n2_max = n2_max;
    m.a_sq = a_sq; m.b_sq = b_sq; m.used = nullptr; m.used_pitch = 0;
    hipLaunchKernelGGL(sqnorm_many_kernel, dim3(aff_cdiv(n1_max > n2_max ? n1_max : n2_max, 4), (unsigned)n_pairs, 2), dim3(256), 0, st, m, dim);
}

// grid (n1_max / 64, P); masked != 0: the second pass, over the columns that are nobody's nearest neighbour in THIS pair
template <int DIM>
__global__ __launch_bounds__(256) void rowmin_many_kernel(SnnMany m, int masked, float* __restrict__ out_min, int32_t* __restrict__ out_idx) {
    __shared__ __attribute__((aligned(16))) float s_b[2 * 16 * ROWMIN_BS(DIM)];
    const int p = blockIdx.y;
    AffPairRow r;
    if (!snn_many_row(m, p, r)) return;
    rowmin_dist_body<DIM, true>(m.desc1 + (size_t)r.row1 * DIM, r.n1, m.desc2 + (size_t)r.row2 * DIM, r.n2, m.a_sq + (size_t)p * m.n1_max,
                          m.b_sq + (size_t)p * m.n2_max, masked ? m.used + (size_t)p * m.used_pitch : (const uint8_t*)nullptr,
                          out_min + (size_t)p * m.n1_max, out_idx + (size_t)p * m.n1_max, (float*)nullptr, blockIdx.x, s_b);
}

// grid (n1_max / 256, P)
__global__ __launch_bounds__(256) void mark_used_many_kernel(SnnMany m, const int32_t* __restrict__ idx) {
    const int p = blockIdx.y;
    AffPairRow r;
    if (!snn_many_row(m, p, r)) return;
    mark_used_body(idx + (size_t)p * m.n1_max, r.n1, m.used + (size_t)p * m.used_pitch, blockIdx.x);
}

// grid (P)
__global__ __launch_bounds__(1024) void snn_select_many_kernel(SnnMany m, const float* __restrict__ min1, const float* __restrict__ min2,
                                                               const int32_t* __restrict__ idx, float thr, int32_t* __restrict__ tent,
                                                               int32_t* __restrict__ count) {
    const int p = blockIdx.x;
    AffPairRow r;
    if (!snn_many_row(m, p, r)) return;
    const size_t o = (size_t)p * m.n1_max;
    snn_select_body(min1 + o, min2 + o, idx + o, r.n1, thr, tent + 2 * o, count + p);
}

// scratch: a_sq float (P, n1_max) | b_sq float (P, n2_max) | used uint8 (P, align16(n2_max)) | second-pass argmin int32 (P, n1_max)
extern "C" size_t affnet_match_many_scratch_bytes(int n_pairs, int n1_max, int n2_max) {
    const size_t P = n_pairs > 0 ? (size_t)n_pairs : 0, a = n1_max > 0 ? (size_t)n1_max : 0, b = n2_max > 0 ? (size_t)n2_max : 0;
    return P * ((a + b) * sizeof(float) + aff_align(b, 16) + a * sizeof(int32_t)) + 64;
}

extern "C" int affnet_match_snn_many(affnet_ctx* ctx, const float* d_desc1, int rows1, const float* d_desc2, int rows2, int dim, const int32_t* d_pairs,
                                     int n_pairs, int n1_max, int n2_max, float snn_threshold, float* d_min_dist, int32_t* d_idx, float* d_min2_dist,
                                     int32_t* d_tent, int32_t* d_count, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_desc1 || !d_desc2 || !d_pairs || !d_min_dist || !d_idx || !d_min2_dist || !d_tent || !d_count || !d_scratch || rows1 < 0 || rows2 < 0 ||
        n_pairs < 0 || n1_max < 0 || n2_max < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "match_snn_many: bad argument");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_snn_many: descriptor length %d (only 128 is built)", dim);
    if (n_pairs > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_snn_many: %d pairs (at most 65535 per call)", n_pairs);
    if (n_pairs == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)n_pairs;
    SnnMany m;
    m.desc1 = d_desc1; m.rows1 = rows1; m.desc2 = d_desc2; m.rows2 = rows2; m.pairs = d_pairs; m.n1_max = n1_max; m.n2_max = n2_max;
    m.a_sq = (float*)d_scratch;
    m.b_sq = m.a_sq + P * n1_max;
    m.used = (uint8_t*)(m.b_sq + P * n2_max);
    m.used_pitch = (int)aff_align((size_t)n2_max, 16);
    int32_t* idx2 = (int32_t*)(m.used + P * m.used_pitch);
    const bool work = n1_max > 0 && n2_max > 0;     // otherwise every pair is empty or out of range
    {
        AffZeroSegs z;
        z.add(d_count, P * sizeof(int32_t));
        if (work) z.add(m.used, P * m.used_pitch);
        int zrc = aff_zero_multi_async(ctx, z, st);
        if (zrc) return zrc;
    }
    if (!work) return AFFNET_OK;
    const unsigned gp = (unsigned)n_pairs;
    hipLaunchKernelGGL(sqnorm_many_kernel, dim3(aff_cdiv(n1_max > n2_max ? n1_max : n2_max, 4), gp, 2), dim3(256), 0, st, m, dim);
    hipLaunchKernelGGL(rowmin_many_kernel<128>, dim3(aff_cdiv(n1_max, 64), gp), dim3(256), 0, st, m, 0, d_min_dist, d_idx);
    hipLaunchKernelGGL(mark_used_many_kernel, dim3(aff_cdiv(n1_max, 256), gp), dim3(256), 0, st, m, (const int32_t*)d_idx);
    hipLaunchKernelGGL(rowmin_many_kernel<128>, dim3(aff_cdiv(n1_max, 64), gp), dim3(256), 0, st, m, 1, d_min2_dist, idx2);
    hipLaunchKernelGGL(snn_select_many_kernel, dim3(gp), dim3(1024), 0, st, m, (const float*)d_min_dist, (const float*)d_min2_dist, (const int32_t*)d_idx,
                       snn_threshold, d_tent, d_count);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// ---- homography reprojection of LAFs + nearest reprojected centre ---------------------------------------------
struct Hom { float h[9]; };

// ReprojectionStuff.py:9-40: centre through H (bmm row-by-column, k ascending), local affine linH at the centre times the
// LAF's 2x2 part.
__global__ void reproject_lafs_kernel(const float* __restrict__ lafs, int n, Hom H, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* L = lafs + 6 * (size_t)i;
    const float x = L[2], y = L[5];
    const float* h = H.h;
    // xy1 = H * [x, y, 1]^T, then / z
    const float X = fmaf(h[2], 1.0f, fmaf(h[1], y, h[0] * x));
    const float Y = fmaf(h[5], 1.0f, fmaf(h[4], y, h[3] * x));
    const float Z = fmaf(h[8], 1.0f, fmaf(h[7], y, h[6] * x));
    // linH (:9-21), operation by operation
    const float den = (x * h[6] + y * h[7]) + h[8];
    const float n1d = ((x * h[0] + y * h[1]) + h[2]) / (den * den);
    const float n2d = ((x * h[3] + y * h[4]) + h[5]) / (den * den);
    const float a00 = h[0] / den - n1d * h[6], a01 = h[1] / den - n1d * h[7];
    const float a10 = h[3] / den - n2d * h[6], a11 = h[4] / den - n2d * h[7];
    float* O = out + 6 * (size_t)i;
    O[0] = fmaf(a01, L[3], a00 * L[0]); O[1] = fmaf(a01, L[4], a00 * L[1]); O[2] = X / Z;
    O[3] = fmaf(a11, L[3], a10 * L[0]); O[4] = fmaf(a11, L[4], a10 * L[1]); O[5] = Y / Z;
}

extern "C" int affnet_reproject_lafs(affnet_ctx* ctx, const float* d_lafs, int n, const float* h_H, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_lafs || !h_H || !d_out || n < 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "reproject_lafs: bad argument");
    if (n == 0) return AFFNET_OK;
    Hom H;
    memcpy(H.h, h_H, sizeof(H.h));
    hipLaunchKernelGGL(reproject_lafs_kernel, dim3(aff_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, d_lafs, n, H, d_out);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// For every query LAF centre (image-1 LAFs): nearest reference centre (the reprojected image-2 LAFs) with
// ReprojectionStuff.py:78-86's own distance_matrix_vector on 2-D points: sqrt(|(|a|^2 + |p|^2) - 2 p.a| + 1e-12) with
// a = reference ("anchor"), p = query ("positive"), in fp32 - at ~800 px coordinates that expansion is only good to
// ~0.1 px, and the 6 px consistency threshold of test() is applied to exactly this value.  ReprojectionStuff.py:126-137.
__global__ void centre_nn_kernel(const float* __restrict__ q, int nq, const float* __restrict__ ref, int nr, float* __restrict__ out_min,
                                 int32_t* __restrict__ out_idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float px = q[6 * (size_t)i + 2], py = q[6 * (size_t)i + 5];
    const float psq = px * px + py * py;
    float best = INFINITY;
    int bi = 0;
    for (int j = 0; j < nr; ++j) {
        const float ax = ref[6 * (size_t)j + 2], ay = ref[6 * (size_t)j + 5];
        const float asq = ax * ax + ay * ay;
        const float dot = fmaf(py, ay, px * ax);
        const float d = sqrtf(fabsf((asq + psq) - 2.0f * dot) + 1e-12f);
        if (d < best) { best = d; bi = j; }
    }
    out_min[i] = best; out_idx[i] = bi;
}

extern "C" int affnet_centre_nn(affnet_ctx* ctx, const float* d_query_lafs, int nq, const float* d_ref_lafs, int nr, float* d_min_dist,
                                int32_t* d_idx, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_query_lafs || !d_ref_lafs || !d_min_dist || !d_idx || nq < 0 || nr < 1)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "centre_nn: bad argument");
    if (nq == 0) return AFFNET_OK;
    hipLaunchKernelGGL(centre_nn_kernel, dim3(aff_cdiv(nq, 128)), dim3(128), 0, (hipStream_t)stream, d_query_lafs, nq, d_ref_lafs, nr, d_min_dist,
                       d_idx);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
