// Guided matching for gfx950: the descriptors are searched again under a verified model, every keypoint among
// the keypoints of the other image that the model allows.  include/affnet_hip.h states the rule in full (affnet_match_guided).
//
// The distance is the matcher's (match.hip, rowmin_dist_body): the same squared-norm kernel (aff_sqnorm_launch), the same chain of
// v_mfma_f32_16x16x4_f32 over the same K order, sqrtf(((asq + bsq) - 2 acc) + 1e-6f) - the element affnet_distance_matrix writes, bit for bit.
// The tile loop is knn_tile_kernel's (knn.hip) restated with two changes: the list holds two candidates (one in the backward pass), and a
// per-pair geometric test stands where the skip range stood.  The order of candidates, the register lists and their merge over lanes are
// topk.h's; the merge over the column chunks is knn.hip's own kernel (aff_knn_merge_launch).
//
// The per-point terms of the geometric test are computed once (guided_prep_kernel) and read by the forward pass, the backward pass and the
// mask kernel through ONE function (guided_ok), so the three cannot disagree about a pair.  -ffp-contract=off: one rounding per operation.
//
// affnet_match_guided_many (end of the file) runs the same stages for P image pairs per launch: guided_many_*_kernel take the pair index from
// the grid, find the pair's segments in a device table and call the bodies of the kernels below, each pair under its own model and gate.
#include <math.h>

#include "common.h"
#include "topk.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define GUIDED_BS(DIM) ((DIM) + 4)    // floats per staged column (knn.hip KNN_BS)
#define GUIDED_WG_PER_CU 3            // chunk choice: workgroups per CU the grid aims at (knn.hip)
#define GUIDED_MIN_TILES 5            // chunk choice: no chunk below this many 16-column tiles (knn.hip)
#define GUIDED_MAX_CHUNKS 1024

// Per-point terms, one float4 per point.
//   planar    image 1: (px, py, W > 0 ? 1 : 0, -)   image 2: (u, v, -, -)
//   epipolar  image 1: (l0, l1, l2, -)              image 2: (u, v, m0, m1)
// grid (cdiv(max(n1, n2), 256), 2): blockIdx.y = 0 image 1, 1 image 2
// The *_body functions are the kernels of one image pair; the __global__ kernels, single-pair here and batched at the end of the file (pair index on
// a grid dimension), only choose the pointers and the workgroup indices they run on.
template <int KIND>
__device__ __forceinline__ void guided_prep_body(const float* __restrict__ lafs1, int n1, const float* __restrict__ lafs2, int n2,
                                                 const double* __restrict__ model, float4* __restrict__ p1, float4* __restrict__ p2, int blk, int side) {
    const int i = blk * 256 + threadIdx.x;
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = (float)model[k];
    if (side == 0) {
        if (i >= n1) return;
        const float x = lafs1[6 * (size_t)i + 2], y = lafs1[6 * (size_t)i + 5];
        if (KIND == AFFNET_GUIDED_PLANAR) {
            const float X = (m[0] * x + m[1] * y) + m[2], Y = (m[3] * x + m[4] * y) + m[5], W = (m[6] * x + m[7] * y) + m[8];
            p1[i] = make_float4(X / W, Y / W, W > 0.0f ? 1.0f : 0.0f, 0.0f);
        } else {
            const float l0 = (m[0] * x + m[1] * y) + m[2], l1 = (m[3] * x + m[4] * y) + m[5], l2 = (m[6] * x + m[7] * y) + m[8];
            p1[i] = make_float4(l0, l1, l2, 0.0f);
        }
    } else {
        if (i >= n2) return;
        const float u = lafs2[6 * (size_t)i + 2], v = lafs2[6 * (size_t)i + 5];
        if (KIND == AFFNET_GUIDED_PLANAR) {
            p2[i] = make_float4(u, v, 0.0f, 0.0f);
        } else {
            const float m0 = (m[0] * u + m[3] * v) + m[6], m1 = (m[1] * u + m[4] * v) + m[7];
            p2[i] = make_float4(u, v, m0, m1);
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void guided_prep_kernel(const float* __restrict__ lafs1, int n1, const float* __restrict__ lafs2, int n2,
                                                          const double* __restrict__ model, float4* __restrict__ p1, float4* __restrict__ p2) {
    guided_prep_body<KIND>(lafs1, n1, lafs2, n2, model, p1, p2, blockIdx.x, blockIdx.y);
}

// The admissible test of the pair (image-1 point with terms a, image-2 point with terms b).  Epipolar: epi_inlier's tree (epipolar.hip).
// A NaN anywhere makes the comparison false.
template <int KIND>
__device__ __forceinline__ bool guided_ok(const float4 a, const float4 b, float r2) {
    if (KIND == AFFNET_GUIDED_PLANAR) {
        const float dx = a.x - b.x, dy = a.y - b.y;
        return a.z > 0.0f && (dx * dx + dy * dy) <= r2;
    }
    const float l0 = a.x, l1 = a.y, l2 = a.z, u = b.x, v = b.y, m0 = b.z, m1 = b.w;
    const float r = (u * l0 + v * l1) + l2;
    const float e = (r * r) / (((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1);
    return e <= r2;
}

// (n1, n2) uint8, one thread per pair
template <int KIND>
__global__ __launch_bounds__(256) void guided_mask_kernel(const float4* __restrict__ p1, int n1, const float4* __restrict__ p2, int n2, float r2,
                                                          uint8_t* __restrict__ mask) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n1 * n2) return;
    const int i = (int)(e / n2), j = (int)(e - (long long)i * n2);
    mask[e] = guided_ok<KIND>(p1[i], p2[j], r2) ? 1 : 0;
}

// The first k of the union of the lists of W lanes (knn.hip, knn_lanes_store)
template <int W, int CAP>
__device__ __forceinline__ void guided_lanes_store(TopkList<float, CAP>& L, bool writer, float* __restrict__ out_d, int32_t* __restrict__ out_i) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        float bd;
        int bi;
        topk_lanes_next<W>(L, bd, bi);
        if (writer) { out_d[j] = bd; out_i[j] = bi == TOPK_EMPTY ? -1 : bi; }
    }
}

// knn_tile_kernel (knn.hip) with CAP candidates per row and the admissible test in place of the skip range.  grid (cdiv(n1, 64), n_chunks);
// rows = `a` with the terms ta, columns = `b` with the terms tb.  SWAP: the backward pass - the rows are image 2, the columns image 1, and
// the test takes its arguments in the forward pass's order.  Each lane holds the terms of its four rows in registers and loads the terms of
// its one column per tile, in front of the MFMAs.  gate != NULL and gate[3] & 1: no tile is walked, every list stays unfilled.
// out_d / out_i: (n1, n_chunks, CAP).
template <int KIND, int CAP, bool SWAP>
__device__ __forceinline__ void guided_tile_body(const float* __restrict__ a, int n1, const float* __restrict__ b, int n2,
                                                 const float* __restrict__ a_sq, const float* __restrict__ b_sq,
                                                 const float4* __restrict__ ta, const float4* __restrict__ tb, float r2,
                                                 const int32_t* __restrict__ gate, int tpc, float* __restrict__ out_d,
                                                 int32_t* __restrict__ out_i, int blk, int chunk, int n_chunks) {
    constexpr int DIM = 128;
    constexpr int NG = DIM / 16;
    constexpr int BS = GUIDED_BS(DIM), Q = DIM / 4, NPRE = 16 * Q / 256;
    static_assert((16 * Q) % 256 == 0, "the staged tile is loaded by 256 threads in whole rounds");
    __shared__ __attribute__((aligned(16))) float s_b[2 * 16 * BS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 15, kq = lane >> 4;
    const int row0 = blk * 64 + wave * 16;
    const int tiles = (n2 + 15) >> 4;
    const long long t0l = (long long)chunk * tpc;
    const bool closed = gate && (gate[3] & 1);                                            // uniform over the grid
    const int t0 = t0l < tiles ? (int)t0l : tiles, t1 = closed ? t0 : min(tiles, t0 + tpc);          // uniform over the workgroup
    TopkList<float, CAP> L[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) L[r].clear();
    if (t0 < t1) {
        f32x4 fa[NG];
        {
            const int r = min(row0 + m, n1 - 1);
#pragma unroll
            for (int t = 0; t < NG; ++t) fa[t] = *reinterpret_cast<const f32x4*>(&a[(size_t)r * DIM + 16 * t + 4 * kq]);
        }
        float asq[4];
        float4 rt[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = min(row0 + 4 * kq + r, n1 - 1);
            asq[r] = a_sq[row];
            rt[r] = ta[row];
        }
        float bound[4] = {INFINITY, INFINITY, INFINITY, INFINITY};      // per row: no candidate behind it can reach the row's list
        f32x4 pre[NPRE];
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
        tile_fetch(16 * t0);
        tile_store(0);
        __syncthreads();
        for (int t = t0; t < t1; ++t) {
            const int c0 = 16 * t;
            const int col = c0 + m;
            const int cc = min(col, n2 - 1);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            f32x4 fb[NG];
            const int buf = (t - t0) & 1;
            const bool more = t + 1 < t1;
            if (more) tile_fetch(c0 + 16);
            // in front of the MFMAs, and no branch between the last MFMA and the accumulator reads (match.hip, NOTES.md)
            const float bsq = b_sq[cc];
            const float4 ct = tb[cc];
            bool cand[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) cand[r] = col < n2 && (SWAP ? guided_ok<KIND>(ct, rt[r], r2) : guided_ok<KIND>(rt[r], ct, r2));
#pragma unroll
            for (int g = 0; g < NG; ++g) fb[g] = *reinterpret_cast<const f32x4*>(&s_b[buf * 16 * BS + m * BS + 16 * g + 4 * kq]);
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[g][j], fb[g][j], acc, 0, 0, 0);
            float d[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = sqrtf(((asq[r] + bsq) - 2.0f * acc[r]) + 1e-6f);      // Losses.py:12-13
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (cand[r] && !(d[r] > bound[r]) && !(d[r] > L[r].d[CAP - 1])) L[r].insert(d[r], col);
            }
            // the row's CAP-th candidate over its 16 lanes becomes the bound after 8, 16, 32, ... tiles, then every 256 (knn.hip)
            const int seen = t - t0 + 1;
            if (seen >= 8 && ((seen & (seen - 1)) == 0 || (seen & 255) == 0)) {
#pragma unroll
                for (int r = 0; r < 4; ++r) bound[r] = topk_lanes_kth<16>(L[r], CAP);
            }
            if (more) tile_store(buf ^ 1);      // the other buffer was last read one tile ago, in front of that tile's barrier
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = min(row0 + 4 * kq + r, n1 - 1);
        const size_t o = ((size_t)row * n_chunks + chunk) * CAP;
        guided_lanes_store<16>(L[r], m == 0 && row0 + 4 * kq + r < n1, out_d + o, out_i + o);
    }
}

template <int KIND, int CAP, bool SWAP>
__global__ __launch_bounds__(256) void guided_tile_kernel(const float* __restrict__ a, int n1, const float* __restrict__ b, int n2,
                                                          const float* __restrict__ a_sq, const float* __restrict__ b_sq,
                                                          const float4* __restrict__ ta, const float4* __restrict__ tb, float r2,
                                                          const int32_t* __restrict__ gate, int tpc, float* __restrict__ out_d,
                                                          int32_t* __restrict__ out_i) {
    guided_tile_body<KIND, CAP, SWAP>(a, n1, b, n2, a_sq, b_sq, ta, tb, r2, gate, tpc, out_d, out_i, blockIdx.x, blockIdx.y, gridDim.y);
}

// One workgroup: the selection rule + order-preserving compaction (match.hip, snn_select_body).  dist / idx: (n1, 2); back: (n2) or NULL.
__device__ __forceinline__ void guided_select_body(const float* __restrict__ dist, const int32_t* __restrict__ idx,
                                                   const int32_t* __restrict__ back, int n1, float thr, float max_dist,
                                                   int32_t* __restrict__ tent, int32_t* __restrict__ count) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i0 = 0; i0 < n1; i0 += 1024) {
        const int i = i0 + threadIdx.x;
        bool keep = false;
        int j = -1;
        if (i < n1) {
            j = idx[2 * (size_t)i];
            const float d0 = dist[2 * (size_t)i], d1 = dist[2 * (size_t)i + 1];
            keep = j >= 0 && d0 <= max_dist && (d0 / (d1 + 1e-8f)) <= thr;
            if (keep && back) keep = back[j] == i;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (keep) {
            const int slot = off + __popcll(bal & ((1ull << lane) - 1ull));
            tent[2 * slot] = i; tent[2 * slot + 1] = j;
        }
        __syncthreads();
        if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += s_wave[w]; s_base += t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = s_base;
}

__global__ __launch_bounds__(1024) void guided_select_kernel(const float* __restrict__ dist, const int32_t* __restrict__ idx,
                                                             const int32_t* __restrict__ back, int n1, float thr, float max_dist,
                                                             int32_t* __restrict__ tent, int32_t* __restrict__ count) {
    guided_select_body(dist, idx, back, n1, thr, max_dist, tent, count);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// the most chunks the library chooses for `cols` columns (aff_chunk_choice never goes above units / min_units)
static size_t guided_most_chunks(size_t cols) {
    const size_t most = ((cols + 15) / 16) / GUIDED_MIN_TILES;
    return most < 1 ? 1 : (most > GUIDED_MAX_CHUNKS ? GUIDED_MAX_CHUNKS : most);
}

// `pairs` searches of `rows` x `cols` each share the part: the grid's row blocks are theirs together
static int guided_chunks(const affnet_ctx* ctx, int rows, int cols, int n_chunks, int pairs = 1) {
    if (n_chunks) return n_chunks;
    return aff_chunk_choice(ctx, (long long)pairs * (rows > 0 ? aff_cdiv(rows, 64) : 1), cols > 0 ? ((long long)cols + 15) / 16 : 0, GUIDED_WG_PER_CU,
                            GUIDED_MIN_TILES, GUIDED_MAX_CHUNKS);
}

// scratch: terms of image 1 float4 (n1) | terms of image 2 float4 (n2) | a_sq float (n1) | b_sq float (n2) | back distance float (n2) |
// back row int32 (n2) | partial distances float | partial rows int32 - the partial lists of the larger of (n1, chunks, 2) and (n2, chunks, 1)
static size_t guided_head_bytes(size_t n1, size_t n2) { return (n1 + n2) * sizeof(float4) + aff_align((n1 + 3 * n2) * sizeof(float), 16); }

extern "C" size_t affnet_match_guided_scratch_bytes(int n1, int n2, int n_chunks) {
    const size_t a = n1 > 0 ? (size_t)n1 : 0, b = n2 > 0 ? (size_t)n2 : 0;
    const size_t ncf = n_chunks > 0 ? (size_t)n_chunks : (n_chunks == 0 ? guided_most_chunks(b) : 0);
    const size_t ncb = n_chunks > 0 ? (size_t)n_chunks : (n_chunks == 0 ? guided_most_chunks(a) : 0);
    const size_t fwd = a * ncf * 2, bwd = b * ncb;
    return guided_head_bytes(a, b) + (fwd > bwd ? fwd : bwd) * (sizeof(float) + sizeof(int32_t)) + 64;
}

static bool guided_radius_ok(float r) { return r > 0.0f && r <= 3.402823466e38f; }

template <int KIND>
static void guided_prep_launch(hipStream_t st, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const double* d_model, float4* p1, float4* p2) {
    hipLaunchKernelGGL(guided_prep_kernel<KIND>, dim3(aff_cdiv(n1 > n2 ? n1 : n2, 256), 2), dim3(256), 0, st, d_lafs1, n1, d_lafs2, n2, d_model, p1, p2);
}

extern "C" int affnet_guided_mask(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const double* d_model, int kind,
                                  float radius, uint8_t* d_mask, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_lafs1 || !d_lafs2 || !d_model || !d_mask || !d_scratch || n1 < 0 || n2 < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "guided_mask: bad argument");
    if (kind != AFFNET_GUIDED_PLANAR && kind != AFFNET_GUIDED_EPIPOLAR) return aff_fail(ctx, AFFNET_ERR_INVALID, "guided_mask: kind %d", kind);
    if (!guided_radius_ok(radius)) return aff_fail(ctx, AFFNET_ERR_INVALID, "guided_mask: the radius must be finite and > 0");
    if (n1 == 0 || n2 == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    float4* p1 = (float4*)d_scratch;
    float4* p2 = p1 + n1;
    const float r2 = radius * radius;
    const long long pairs = (long long)n1 * n2;
    const unsigned blocks = (unsigned)((pairs + 255) / 256);
    if (kind == AFFNET_GUIDED_PLANAR) {
        guided_prep_launch<AFFNET_GUIDED_PLANAR>(st, d_lafs1, n1, d_lafs2, n2, d_model, p1, p2);
        hipLaunchKernelGGL(guided_mask_kernel<AFFNET_GUIDED_PLANAR>, dim3(blocks), dim3(256), 0, st, (const float4*)p1, n1, (const float4*)p2, n2, r2, d_mask);
    } else {
        guided_prep_launch<AFFNET_GUIDED_EPIPOLAR>(st, d_lafs1, n1, d_lafs2, n2, d_model, p1, p2);
        hipLaunchKernelGGL(guided_mask_kernel<AFFNET_GUIDED_EPIPOLAR>, dim3(blocks), dim3(256), 0, st, (const float4*)p1, n1, (const float4*)p2, n2, r2, d_mask);
    }
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

struct GuidedCall {
    const float* d1; int n1; const float* d2; int n2;
    const float* a_sq; const float* b_sq; const float4* p1; const float4* p2;
    float r2; const int32_t* gate;
    int ncf, ncb;                                  // chunks of the forward / the backward pass
    float* part_d; int32_t* part_i;
    float* dist; int32_t* idx;                     // (n1, 2)
    float* back_d; int32_t* back_i;                // (n2), or NULL: no backward pass
};

// forward pass (+ merge), backward pass (+ merge)
template <int KIND>
static void guided_passes_launch(hipStream_t st, const GuidedCall& c) {
    {
        const int tpc = aff_cdiv(aff_cdiv(c.n2, 16), c.ncf);
        float* td = c.ncf == 1 ? c.dist : c.part_d;
        int32_t* ti = c.ncf == 1 ? c.idx : c.part_i;
        hipLaunchKernelGGL((guided_tile_kernel<KIND, 2, false>), dim3(aff_cdiv(c.n1, 64), c.ncf), dim3(256), 0, st, c.d1, c.n1, c.d2, c.n2, c.a_sq, c.b_sq,
                           c.p1, c.p2, c.r2, c.gate, tpc, td, ti);
        if (c.ncf > 1) aff_knn_merge_launch(st, c.part_d, c.part_i, c.n1, c.ncf, 2, c.dist, c.idx);
    }
    if (c.back_i && c.n2 > 0) {
        const int tpc = aff_cdiv(aff_cdiv(c.n1, 16), c.ncb);
        float* td = c.ncb == 1 ? c.back_d : c.part_d;
        int32_t* ti = c.ncb == 1 ? c.back_i : c.part_i;
        hipLaunchKernelGGL((guided_tile_kernel<KIND, 1, true>), dim3(aff_cdiv(c.n2, 64), c.ncb), dim3(256), 0, st, c.d2, c.n2, c.d1, c.n1, c.b_sq, c.a_sq,
                           c.p2, c.p1, c.r2, c.gate, tpc, td, ti);
        if (c.ncb > 1) aff_knn_merge_launch(st, c.part_d, c.part_i, c.n2, c.ncb, 1, c.back_d, c.back_i);
    }
}

extern "C" int affnet_match_guided(affnet_ctx* ctx, const float* d_desc1, int n1, const float* d_desc2, int n2, int dim, const float* d_lafs1,
                                   const float* d_lafs2, const double* d_model, int kind, float radius, float snn_threshold, float max_dist,
                                   int flags, int n_chunks, const int32_t* d_gate, float* d_dist, int32_t* d_idx, int32_t* d_tent,
                                   int32_t* d_count, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_desc1 || !d_desc2 || !d_lafs1 || !d_lafs2 || !d_model || !d_dist || !d_idx || !d_tent || !d_count || !d_scratch || n1 < 0 || n2 < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided: bad argument");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided: descriptor length %d (only 128 is built)", dim);
    if (kind != AFFNET_GUIDED_PLANAR && kind != AFFNET_GUIDED_EPIPOLAR) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided: kind %d", kind);
    if (flags & ~AFFNET_GUIDED_MUTUAL) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided: flags %d", flags);
    if (!guided_radius_ok(radius)) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided: the radius must be finite and > 0");
    if (max_dist != max_dist) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided: max_dist is NaN");
    if (n_chunks < 0 || n_chunks > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided: %d chunks (0..65535)", n_chunks);
    hipStream_t st = (hipStream_t)stream;
    if (n1 == 0) return aff_zero_async(ctx, d_count, sizeof(int32_t), st);
    const bool mutual = (flags & AFFNET_GUIDED_MUTUAL) != 0;
    GuidedCall c;
    c.d1 = d_desc1; c.n1 = n1; c.d2 = d_desc2; c.n2 = n2;
    float4* p1 = (float4*)d_scratch;
    float4* p2 = p1 + n1;
    float* a_sq = (float*)(p2 + n2);
    float* b_sq = a_sq + n1;
    c.p1 = p1; c.p2 = p2; c.a_sq = a_sq; c.b_sq = b_sq;
    c.back_d = mutual ? b_sq + n2 : nullptr;
    c.back_i = mutual ? (int32_t*)(b_sq + 2 * (size_t)n2) : nullptr;
    c.ncf = guided_chunks(ctx, n1, n2, n_chunks);
    c.ncb = guided_chunks(ctx, n2, n1, n_chunks);
    const size_t fwd = (size_t)n1 * c.ncf * 2, bwd = (size_t)n2 * c.ncb;
    c.part_d = (float*)((char*)d_scratch + guided_head_bytes((size_t)n1, (size_t)n2));
    c.part_i = (int32_t*)(c.part_d + (fwd > bwd ? fwd : bwd));
    c.r2 = radius * radius; c.gate = d_gate; c.dist = d_dist; c.idx = d_idx;
    aff_sqnorm_launch(st, d_desc1, n1, dim, a_sq);
    aff_sqnorm_launch(st, d_desc2, n2, dim, b_sq);
    if (kind == AFFNET_GUIDED_PLANAR) {
        guided_prep_launch<AFFNET_GUIDED_PLANAR>(st, d_lafs1, n1, d_lafs2, n2, d_model, p1, p2);
        guided_passes_launch<AFFNET_GUIDED_PLANAR>(st, c);
    } else {
        guided_prep_launch<AFFNET_GUIDED_EPIPOLAR>(st, d_lafs1, n1, d_lafs2, n2, d_model, p1, p2);
        guided_passes_launch<AFFNET_GUIDED_EPIPOLAR>(st, c);
    }
    hipLaunchKernelGGL(guided_select_kernel, dim3(1), dim3(1024), 0, st, (const float*)d_dist, (const int32_t*)d_idx, (const int32_t*)c.back_i, n1,
                       snn_threshold, max_dist, d_tent, d_count);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// ---- many pairs in one call: the pair index on a grid dimension of every stage --------------------------------------------------------------
// One pair of 2000 x 2000 is 32 row blocks on 256 CUs and a chain of short launches; P pairs are P x the workgroups in the same launches.  Every
// kernel reads its row of the pair table, tests it (aff_pair_row, before any load through it) and runs the single-pair body above on the pair's
// segments under the pair's own model row and gate row: per pair the outputs are affnet_match_guided's bit for bit.  The chunk count is one per
// launch (from the caps), which the result does not depend on; a chunk past a pair's own columns leaves unfilled lists for the merge.
struct GuidedMany {
    const float* desc1; int rows1;
    const float* desc2; int rows2;
    const float* lafs1; const float* lafs2;
    const int32_t* pairs;
    int n1_max, n2_max;
    const double* model;               // (P, 9)
    const int32_t* gate;               // (P, 4) or NULL
    float4* p1; float4* p2;            // scratch: (P, n1_max), (P, n2_max)
    float* a_sq; float* b_sq;          // scratch: (P, n1_max), (P, n2_max)
    float* back_d; int32_t* back_i;    // scratch: (P, n2_max)
};

// false: the row is out of range, or image 1 of the pair is empty - nothing to do either way (d_count was cleared)
__device__ __forceinline__ bool guided_many_row(const GuidedMany& g, int p, AffPairRow& r) {
    return aff_pair_row(g.pairs, p, g.rows1, g.rows2, g.n1_max, g.n2_max, r) && r.n1 > 0;
}

// grid (cdiv(max(n1_max, n2_max), 256), 2, P)
template <int KIND>
__global__ __launch_bounds__(256) void guided_many_prep_kernel(GuidedMany g) {
    const int p = blockIdx.z;
    AffPairRow r;
    if (!guided_many_row(g, p, r)) return;
    guided_prep_body<KIND>(g.lafs1 + 6 * (size_t)r.row1, r.n1, g.lafs2 + 6 * (size_t)r.row2, r.n2, g.model + 9 * (size_t)p, g.p1 + (size_t)p * g.n1_max,
                           g.p2 + (size_t)p * g.n2_max, blockIdx.x, blockIdx.y);
}

// grid (cdiv(rows_max, 64), n_chunks, P), rows = image 1 (forward) or, SWAP, image 2 (backward: a pair without rows in image 2 has no backward
// pass).  out_d / out_i: (P, rows_max, n_chunks, CAP).
template <int KIND, int CAP, bool SWAP>
__global__ __launch_bounds__(256) void guided_many_tile_kernel(GuidedMany g, float r2, int tpc, float* __restrict__ out_d, int32_t* __restrict__ out_i) {
    const int p = blockIdx.z;
    AffPairRow r;
    if (!guided_many_row(g, p, r)) return;
    if (SWAP && r.n2 == 0) return;
    const float* d1 = g.desc1 + 128 * (size_t)r.row1;
    const float* d2 = g.desc2 + 128 * (size_t)r.row2;
    const size_t o1 = (size_t)p * g.n1_max, o2 = (size_t)p * g.n2_max;
    const int32_t* gate = g.gate ? g.gate + 4 * (size_t)p : nullptr;
    const size_t o = (SWAP ? o2 : o1) * gridDim.y * CAP;
    if (SWAP)
        guided_tile_body<KIND, CAP, true>(d2, r.n2, d1, r.n1, g.b_sq + o2, g.a_sq + o1, g.p2 + o2, g.p1 + o1, r2, gate, tpc, out_d + o, out_i + o, blockIdx.x,
                                          blockIdx.y, gridDim.y);
    else
        guided_tile_body<KIND, CAP, false>(d1, r.n1, d2, r.n2, g.a_sq + o1, g.b_sq + o2, g.p1 + o1, g.p2 + o2, r2, gate, tpc, out_d + o, out_i + o, blockIdx.x,
                                           blockIdx.y, gridDim.y);
}

// grid (P).  dist / idx: (P, n1_max, 2); tent (P, n1_max, 2); count (P)
__global__ __launch_bounds__(1024) void guided_many_select_kernel(GuidedMany g, const float* __restrict__ dist, const int32_t* __restrict__ idx, int mutual,
                                                                  float thr, float max_dist, int32_t* __restrict__ tent, int32_t* __restrict__ count) {
    const int p = blockIdx.x;
    AffPairRow r;
    if (!guided_many_row(g, p, r)) return;
    const size_t o = (size_t)p * g.n1_max;
    guided_select_body(dist + 2 * o, idx + 2 * o, mutual ? g.back_i + (size_t)p * g.n2_max : (const int32_t*)nullptr, r.n1, thr, max_dist, tent + 2 * o,
                       count + p);
}

// scratch: terms of image 1 float4 (P, n1_max) | terms of image 2 float4 (P, n2_max) | a_sq float (P, n1_max) | b_sq float (P, n2_max) |
// back distance float (P, n2_max) | back row int32 (P, n2_max) | partial distances float | partial rows int32 - the partial lists of the larger of
// (P, n1_max, chunks, 2) and (P, n2_max, chunks, 1)
extern "C" size_t affnet_match_guided_many_scratch_bytes(int n_pairs, int n1_max, int n2_max, int n_chunks) {
    const size_t P = n_pairs > 0 ? (size_t)n_pairs : 0, a = n1_max > 0 ? (size_t)n1_max : 0, b = n2_max > 0 ? (size_t)n2_max : 0;
    const size_t ncf = n_chunks > 0 ? (size_t)n_chunks : (n_chunks == 0 ? guided_most_chunks(b) : 0);
    const size_t ncb = n_chunks > 0 ? (size_t)n_chunks : (n_chunks == 0 ? guided_most_chunks(a) : 0);
    const size_t fwd = a * ncf * 2, bwd = b * ncb;
    return P * (guided_head_bytes(a, b) + (fwd > bwd ? fwd : bwd) * (sizeof(float) + sizeof(int32_t))) + 64;
}

template <int KIND>
static void guided_many_launch(hipStream_t st, const GuidedMany& g, int n_pairs, float r2, int ncf, int ncb, bool mutual, float* part_d, int32_t* part_i,
                               float* d_dist, int32_t* d_idx) {
    const unsigned gp = (unsigned)n_pairs;
    const int n1 = g.n1_max, n2 = g.n2_max;
    hipLaunchKernelGGL(guided_many_prep_kernel<KIND>, dim3(aff_cdiv(n1 > n2 ? n1 : n2, 256), 2, gp), dim3(256), 0, st, g);
    {
        const int tpc = aff_cdiv(aff_cdiv(n2, 16), ncf);
        hipLaunchKernelGGL((guided_many_tile_kernel<KIND, 2, false>), dim3(aff_cdiv(n1, 64), ncf, gp), dim3(256), 0, st, g, r2, tpc, ncf == 1 ? d_dist : part_d,
                           ncf == 1 ? d_idx : part_i);
        if (ncf > 1) aff_knn_merge_pairs_launch(st, part_d, part_i, g.pairs, n_pairs, g.rows1, g.rows2, n1, n2, 0, ncf, 2, d_dist, d_idx);
    }
    if (mutual && n2 > 0) {
        const int tpc = aff_cdiv(aff_cdiv(n1, 16), ncb);
        hipLaunchKernelGGL((guided_many_tile_kernel<KIND, 1, true>), dim3(aff_cdiv(n2, 64), ncb, gp), dim3(256), 0, st, g, r2, tpc, ncb == 1 ? g.back_d : part_d,
                           ncb == 1 ? g.back_i : part_i);
        if (ncb > 1) aff_knn_merge_pairs_launch(st, part_d, part_i, g.pairs, n_pairs, g.rows1, g.rows2, n1, n2, 1, ncb, 1, g.back_d, g.back_i);
    }
}

extern "C" int affnet_match_guided_many(affnet_ctx* ctx, const float* d_desc1, int rows1, const float* d_desc2, int rows2, int dim, const float* d_lafs1,
                                        const float* d_lafs2, const int32_t* d_pairs, int n_pairs, int n1_max, int n2_max, const double* d_model, int kind,
                                        float radius, float snn_threshold, float max_dist, int flags, int n_chunks, const int32_t* d_gate, float* d_dist,
                                        int32_t* d_idx, int32_t* d_tent, int32_t* d_count, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_desc1 || !d_desc2 || !d_lafs1 || !d_lafs2 || !d_pairs || !d_model || !d_dist || !d_idx || !d_tent || !d_count || !d_scratch || rows1 < 0 ||
        rows2 < 0 || n_pairs < 0 || n1_max < 0 || n2_max < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: bad argument");
    if (((uintptr_t)d_scratch & 15) != 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: d_scratch must be 16-byte aligned");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: descriptor length %d (only 128 is built)", dim);
    if (n_pairs > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: %d pairs (at most 65535 per call)", n_pairs);
    if (kind != AFFNET_GUIDED_PLANAR && kind != AFFNET_GUIDED_EPIPOLAR) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: kind %d", kind);
    if (flags & ~AFFNET_GUIDED_MUTUAL) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: flags %d", flags);
    if (!guided_radius_ok(radius)) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: the radius must be finite and > 0");
    if (max_dist != max_dist) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: max_dist is NaN");
    if (n_chunks < 0 || n_chunks > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_guided_many: %d chunks (0..65535)", n_chunks);
    if (n_pairs == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)n_pairs, a = (size_t)n1_max, b = (size_t)n2_max;
    { int zrc = aff_zero_async(ctx, d_count, P * sizeof(int32_t), st); if (zrc) return zrc; }
    if (n1_max == 0) return AFFNET_OK;               // image 1 of every pair is empty, or the pair is out of range
    const bool mutual = (flags & AFFNET_GUIDED_MUTUAL) != 0;
    GuidedMany g;
    g.desc1 = d_desc1; g.rows1 = rows1; g.desc2 = d_desc2; g.rows2 = rows2; g.lafs1 = d_lafs1; g.lafs2 = d_lafs2; g.pairs = d_pairs;
    g.n1_max = n1_max; g.n2_max = n2_max; g.model = d_model; g.gate = d_gate;
    g.p1 = (float4*)d_scratch;
    g.p2 = g.p1 + P * a;
    g.a_sq = (float*)(g.p2 + P * b);
    g.b_sq = g.a_sq + P * a;
    g.back_d = g.b_sq + P * b;
    g.back_i = (int32_t*)(g.back_d + P * b);
    const int ncf = guided_chunks(ctx, n1_max, n2_max, n_chunks, n_pairs), ncb = guided_chunks(ctx, n2_max, n1_max, n_chunks, n_pairs);
    const size_t fwd = P * a * ncf * 2, bwd = P * b * ncb;
    float* part_d = (float*)((char*)d_scratch + P * guided_head_bytes(a, b));
    int32_t* part_i = (int32_t*)(part_d + (fwd > bwd ? fwd : bwd));
    const float r2 = radius * radius;
    aff_sqnorm_many_launch(st, d_desc1, rows1, d_desc2, rows2, dim, d_pairs, n_pairs, n1_max, n2_max, g.a_sq, g.b_sq);
    if (kind == AFFNET_GUIDED_PLANAR) guided_many_launch<AFFNET_GUIDED_PLANAR>(st, g, n_pairs, r2, ncf, ncb, mutual, part_d, part_i, d_dist, d_idx);
    else guided_many_launch<AFFNET_GUIDED_EPIPOLAR>(st, g, n_pairs, r2, ncf, ncb, mutual, part_d, part_i, d_dist, d_idx);
    hipLaunchKernelGGL(guided_many_select_kernel, dim3((unsigned)n_pairs), dim3(1024), 0, st, g, (const float*)d_dist, (const int32_t*)d_idx, mutual ? 1 : 0,
                       snn_threshold, max_dist, d_tent, d_count);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
