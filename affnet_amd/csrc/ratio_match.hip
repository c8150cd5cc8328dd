// Ratio-test matching for gfx950: per row the nearest column and the second nearest - or, with a radius, the first
// neighbour whose centre is geometrically inconsistent with the nearest one's (FGINN) - the ratio of the two, an optional mutual check.
// include/affnet_hip.h states the rule in full (affnet_match_ratio).
//
// The distance is the matcher's (match.hip, rowmin_dist_body): the same squared-norm kernel (aff_sqnorm_launch), the same chain of
// v_mfma_f32_16x16x4_f32 over the same K order, sqrtf(((asq + bsq) - 2 acc) + 1e-6f) - the element affnet_distance_matrix writes, bit for bit.
// The tile loop is guided_tile_body's (guided.hip) restated without the admissible test.  The order of candidates, the register lists and
// their merge over lanes are topk.h's; the merge over the column chunks is knn.hip's own kernel (aff_knn_merge_launch).
//
// Passes.  radius < 0: one forward pass with lists of two - the whole search.  radius >= 0: a forward pass with lists of one (the nearest
// column j1 of every row), then the FGINN pass: each lane holds j1 and its centre for its four rows and inserts a column only where it is not
// j1 and ratio_inconsistent says so.  This is exact where a list of fixed length is not: nine detections on one place push the first
// inconsistent column out of a list of eight.  MUTUAL: the forward kernel with the sides exchanged, lists of one.  The inconsistency test is
// ONE function; -ffp-contract=off: one rounding per operation.
//
// With a radius the two slots of a row come from two passes, so they lie in two scratch arrays and the selection kernel, which reads them
// anyway, writes them to (n1, 2) d_dist / d_idx.
//
// affnet_match_ratio_many (end of the file) runs the same stages for P image pairs per launch: ratio_many_*_kernel take the pair index from
// the grid, find the pair's segments in a device table and call the bodies of the kernels below.
#include <math.h>

#include "common.h"
#include "topk.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define RATIO_BS(DIM) ((DIM) + 4)    // floats per staged column (knn.hip KNN_BS)
#define RATIO_WG_PER_CU 3            // chunk choice: workgroups per CU the grid aims at (knn.hip)
#define RATIO_MIN_TILES 5            // chunk choice: no chunk below this many 16-column tiles (knn.hip)
#define RATIO_MAX_CHUNKS 1024

// Column with centre (u, v) against the nearest column's centre (u1, v1): not within the radius.  A NaN anywhere makes the comparison
// false and the column inconsistent.
__device__ __forceinline__ bool ratio_inconsistent(float u, float v, float u1, float v1, float r2) {
    const float du = u - u1, dv = v - v1;
    return !((du * du + dv * dv) <= r2);
}

// The first k of the union of the lists of W lanes (knn.hip, knn_lanes_store)
template <int W, int CAP>
__device__ __forceinline__ void ratio_lanes_store(TopkList<float, CAP>& L, bool writer, float* __restrict__ out_d, int32_t* __restrict__ out_i) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        float bd;
        int bi;
        topk_lanes_next<W>(L, bd, bi);
        if (writer) { out_d[j] = bd; out_i[j] = bi == TOPK_EMPTY ? -1 : bi; }
    }
}

// guided_tile_body (guided.hip) with CAP candidates per row and no admissible test.  grid (cdiv(n1, 64), n_chunks); rows = `a`, columns = `b`.
// FGINN: `first` (n1) holds every row's nearest column j1 and `cen` the frames (n2,2,3) of the columns; each lane gathers j1 and its centre for
// its four rows once, loads the centre of its one column per tile in front of the MFMAs, and a column is a candidate only where it is not
// j1 and inconsistent with it.  out_d / out_i: (n1, n_chunks, CAP).
template <int CAP, bool FGINN>
__device__ __forceinline__ void ratio_tile_body(const float* __restrict__ a, int n1, const float* __restrict__ b, int n2,
                                                const float* __restrict__ a_sq, const float* __restrict__ b_sq,
                                                const float* __restrict__ cen, const int32_t* __restrict__ first, float r2, int tpc,
                                                float* __restrict__ out_d, int32_t* __restrict__ out_i, int blk, int chunk, int n_chunks) {
    constexpr int DIM = 128;
    constexpr int NG = DIM / 16;
    constexpr int BS = RATIO_BS(DIM), Q = DIM / 4, NPRE = 16 * Q / 256;
    static_assert((16 * Q) % 256 == 0, "the staged tile is loaded by 256 threads in whole rounds");
    __shared__ __attribute__((aligned(16))) float s_b[2 * 16 * BS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 15, kq = lane >> 4;
    const int row0 = blk * 64 + wave * 16;
    const int tiles = (n2 + 15) >> 4;
    const long long t0l = (long long)chunk * tpc;
    const int t0 = t0l < tiles ? (int)t0l : tiles, t1 = min(tiles, t0 + tpc);          // uniform over the workgroup
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
        int j1[4];
        float u1[4], v1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = min(row0 + 4 * kq + r, n1 - 1);
            asq[r] = a_sq[row];
            if (FGINN) {
                j1[r] = first[row];
                const int jc = min(max(j1[r], 0), n2 - 1);      // n2 > 0 here, and then every row has a nearest column; the clamp only guards the load
                u1[r] = cen[6 * (size_t)jc + 2];
                v1[r] = cen[6 * (size_t)jc + 5];
            }
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
            bool cand[4];
            if (FGINN) {
                const float cu = cen[6 * (size_t)cc + 2], cv = cen[6 * (size_t)cc + 5];
#pragma unroll
                for (int r = 0; r < 4; ++r) cand[r] = col < n2 && col != j1[r] && ratio_inconsistent(cu, cv, u1[r], v1[r], r2);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) cand[r] = col < n2;
            }
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
        ratio_lanes_store<16>(L[r], m == 0 && row0 + 4 * kq + r < n1, out_d + o, out_i + o);
    }
}

template <int CAP, bool FGINN>
__global__ __launch_bounds__(256) void ratio_tile_kernel(const float* __restrict__ a, int n1, const float* __restrict__ b, int n2,
                                                         const float* __restrict__ a_sq, const float* __restrict__ b_sq,
                                                         const float* __restrict__ cen, const int32_t* __restrict__ first, float r2, int tpc,
                                                         float* __restrict__ out_d, int32_t* __restrict__ out_i) {
    ratio_tile_body<CAP, FGINN>(a, n1, b, n2, a_sq, b_sq, cen, first, r2, tpc, out_d, out_i, blockIdx.x, blockIdx.y, gridDim.y);
}

// One workgroup: the selection rule + order-preserving compaction (match.hip, snn_select_body).  dist / idx: (n1, 2); back: (n2) or NULL.
// PACK: the slots of row i are (d0[i], i0[i]) and (d1[i], i1[i]) and are written to dist / idx here; otherwise dist / idx hold them already.
template <bool PACK>
__device__ __forceinline__ void ratio_select_body(const float* __restrict__ d0s, const int32_t* __restrict__ i0s, const float* __restrict__ d1s,
                                                  const int32_t* __restrict__ i1s, float* __restrict__ dist, int32_t* __restrict__ idx,
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
            float d0, d1;
            if (PACK) {
                j = i0s[i];
                d0 = d0s[i]; d1 = d1s[i];
                dist[2 * (size_t)i] = d0; dist[2 * (size_t)i + 1] = d1;
                idx[2 * (size_t)i] = j; idx[2 * (size_t)i + 1] = i1s[i];
            } else {
                j = idx[2 * (size_t)i];
                d0 = dist[2 * (size_t)i]; d1 = dist[2 * (size_t)i + 1];
            }
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

template <bool PACK>
__global__ __launch_bounds__(1024) void ratio_select_kernel(const float* __restrict__ d0s, const int32_t* __restrict__ i0s, const float* __restrict__ d1s,
                                                            const int32_t* __restrict__ i1s, float* __restrict__ dist, int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ back, int n1, float thr, float max_dist,
                                                            int32_t* __restrict__ tent, int32_t* __restrict__ count) {
    ratio_select_body<PACK>(d0s, i0s, d1s, i1s, dist, idx, back, n1, thr, max_dist, tent, count);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// the most chunks the library chooses for `cols` columns (aff_chunk_choice never goes above units / min_units)
static size_t ratio_most_chunks(size_t cols) {
    const size_t most = ((cols + 15) / 16) / RATIO_MIN_TILES;
    return most < 1 ? 1 : (most > RATIO_MAX_CHUNKS ? RATIO_MAX_CHUNKS : most);
}

// `pairs` searches of `rows` x `cols` each share the part: the grid's row blocks are theirs together.  One pair: affnet_knn_chunks' value.
static int ratio_chunks(const affnet_ctx* ctx, int rows, int cols, int n_chunks, int pairs) {
    if (n_chunks) return n_chunks;
    return aff_chunk_choice(ctx, (long long)pairs * (rows > 0 ? aff_cdiv(rows, 64) : 1), cols > 0 ? ((long long)cols + 15) / 16 : 0, RATIO_WG_PER_CU,
                            RATIO_MIN_TILES, RATIO_MAX_CHUNKS);
}

// scratch: a_sq float (n1) | first distance float (n1) | first column int32 (n1) | second distance float (n1) | second column int32 (n1) |
// b_sq float (n2) | back distance float (n2) | back row int32 (n2) | partial distances float | partial rows int32 - the partial lists of the
// larger of (n1, chunks, 2) and (n2, chunks, 1)
static size_t ratio_head_bytes(size_t n1, size_t n2) { return aff_align((5 * n1 + 3 * n2) * sizeof(float), 16); }

static size_t ratio_part_slots(size_t a, size_t b, int n_chunks) {
    const size_t ncf = n_chunks > 0 ? (size_t)n_chunks : (n_chunks == 0 ? ratio_most_chunks(b) : 0);
    const size_t ncb = n_chunks > 0 ? (size_t)n_chunks : (n_chunks == 0 ? ratio_most_chunks(a) : 0);
    const size_t fwd = a * ncf * 2, bwd = b * ncb;
    return fwd > bwd ? fwd : bwd;
}

extern "C" size_t affnet_match_ratio_scratch_bytes(int n1, int n2, int n_chunks) {
    const size_t a = n1 > 0 ? (size_t)n1 : 0, b = n2 > 0 ? (size_t)n2 : 0;
    return ratio_head_bytes(a, b) + ratio_part_slots(a, b, n_chunks) * (sizeof(float) + sizeof(int32_t)) + 64;
}

// the argument checks the two entry points share; 0 or the error code
static int ratio_args_check(affnet_ctx* ctx, const char* who, int dim, const float* d_lafs2, float radius, float max_dist, int flags, int n_chunks,
                            const void* d_scratch) {
    if (((uintptr_t)d_scratch & 15) != 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: d_scratch must be 16-byte aligned", who);
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: descriptor length %d (only 128 is built)", who, dim);
    if (flags & ~AFFNET_RATIO_MUTUAL) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: flags %d", who, flags);
    if (radius != radius || radius > 3.402823466e38f) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: the radius must not be NaN or +inf", who);
    if (radius >= 0.0f && !d_lafs2) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: a radius >= 0 needs d_lafs2", who);
    if (max_dist != max_dist) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: max_dist is NaN", who);
    if (n_chunks < 0 || n_chunks > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: %d chunks (0..65535)", who, n_chunks);
    return 0;
}

extern "C" int affnet_match_ratio(affnet_ctx* ctx, const float* d_desc1, int n1, const float* d_desc2, int n2, int dim, const float* d_lafs2, float radius,
                                  float snn_threshold, float max_dist, int flags, int n_chunks, float* d_dist, int32_t* d_idx, int32_t* d_tent,
                                  int32_t* d_count, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_desc1 || !d_desc2 || !d_dist || !d_idx || !d_tent || !d_count || !d_scratch || n1 < 0 || n2 < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "match_ratio: bad argument");
    { int rc = ratio_args_check(ctx, "match_ratio", dim, d_lafs2, radius, max_dist, flags, n_chunks, d_scratch); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    if (n1 == 0) return aff_zero_async(ctx, d_count, sizeof(int32_t), st);
    const bool mutual = (flags & AFFNET_RATIO_MUTUAL) != 0, fginn = radius >= 0.0f;
    float* a_sq = (float*)d_scratch;
    float* first_d = a_sq + n1;
    int32_t* first_i = (int32_t*)(first_d + n1);
    float* sec_d = (float*)(first_i + n1);
    int32_t* sec_i = (int32_t*)(sec_d + n1);
    float* b_sq = (float*)(sec_i + n1);
    float* back_d = b_sq + n2;
    int32_t* back_i = (int32_t*)(back_d + n2);
    const int ncf = ratio_chunks(ctx, n1, n2, n_chunks, 1), ncb = ratio_chunks(ctx, n2, n1, n_chunks, 1);
    const size_t fwd = (size_t)n1 * ncf * 2, bwd = (size_t)n2 * ncb;
    float* part_d = (float*)((char*)d_scratch + ratio_head_bytes((size_t)n1, (size_t)n2));
    int32_t* part_i = (int32_t*)(part_d + (fwd > bwd ? fwd : bwd));
    const float r2 = radius * radius;
    const dim3 gf(aff_cdiv(n1, 64), ncf);
    const int tpcf = aff_cdiv(aff_cdiv(n2, 16), ncf);
    aff_sqnorm_launch(st, d_desc1, n1, dim, a_sq);
    aff_sqnorm_launch(st, d_desc2, n2, dim, b_sq);
    if (!fginn) {
        hipLaunchKernelGGL((ratio_tile_kernel<2, false>), gf, dim3(256), 0, st, d_desc1, n1, d_desc2, n2, (const float*)a_sq, (const float*)b_sq,
                           (const float*)nullptr, (const int32_t*)nullptr, 0.0f, tpcf, ncf == 1 ? d_dist : part_d, ncf == 1 ? d_idx : part_i);
        if (ncf > 1) aff_knn_merge_launch(st, part_d, part_i, n1, ncf, 2, d_dist, d_idx);
    } else {
        hipLaunchKernelGGL((ratio_tile_kernel<1, false>), gf, dim3(256), 0, st, d_desc1, n1, d_desc2, n2, (const float*)a_sq, (const float*)b_sq,
                           (const float*)nullptr, (const int32_t*)nullptr, 0.0f, tpcf, ncf == 1 ? first_d : part_d, ncf == 1 ? first_i : part_i);
        if (ncf > 1) aff_knn_merge_launch(st, part_d, part_i, n1, ncf, 1, first_d, first_i);
        hipLaunchKernelGGL((ratio_tile_kernel<1, true>), gf, dim3(256), 0, st, d_desc1, n1, d_desc2, n2, (const float*)a_sq, (const float*)b_sq, d_lafs2,
                           (const int32_t*)first_i, r2, tpcf, ncf == 1 ? sec_d : part_d, ncf == 1 ? sec_i : part_i);
        if (ncf > 1) aff_knn_merge_launch(st, part_d, part_i, n1, ncf, 1, sec_d, sec_i);
    }
    if (mutual && n2 > 0) {
        const int tpc = aff_cdiv(aff_cdiv(n1, 16), ncb);
        hipLaunchKernelGGL((ratio_tile_kernel<1, false>), dim3(aff_cdiv(n2, 64), ncb), dim3(256), 0, st, d_desc2, n2, d_desc1, n1, (const float*)b_sq,
                           (const float*)a_sq, (const float*)nullptr, (const int32_t*)nullptr, 0.0f, tpc, ncb == 1 ? back_d : part_d, ncb == 1 ? back_i : part_i);
        if (ncb > 1) aff_knn_merge_launch(st, part_d, part_i, n2, ncb, 1, back_d, back_i);
    }
    const int32_t* back = mutual ? back_i : nullptr;
    if (fginn)
        hipLaunchKernelGGL(ratio_select_kernel<true>, dim3(1), dim3(1024), 0, st, (const float*)first_d, (const int32_t*)first_i, (const float*)sec_d,
                           (const int32_t*)sec_i, d_dist, d_idx, back, n1, snn_threshold, max_dist, d_tent, d_count);
    else
        hipLaunchKernelGGL(ratio_select_kernel<false>, dim3(1), dim3(1024), 0, st, (const float*)nullptr, (const int32_t*)nullptr, (const float*)nullptr,
                           (const int32_t*)nullptr, d_dist, d_idx, back, n1, snn_threshold, max_dist, d_tent, d_count);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// ---- many pairs in one call: the pair index on a grid dimension of every stage --------------------------------------------------------------
// One pair of 2000 x 2000 is 32 row blocks on 256 CUs and a chain of short launches; P pairs are P x the workgroups in the same launches.  Every
// kernel reads its row of the pair table, tests it (aff_pair_row, before any load through it) and runs the single-pair body above on the pair's
// segments: per pair the outputs are affnet_match_ratio's bit for bit.  The chunk count is one per launch (from the caps), which the result does
// not depend on; a chunk past a pair's own columns leaves unfilled lists for the merge.
struct RatioMany {
    const float* desc1; int rows1;
    const float* desc2; int rows2;
    const float* lafs2;
    const int32_t* pairs;
    int n1_max, n2_max;
    float* a_sq; float* b_sq;                // scratch: (P, n1_max), (P, n2_max)
    float* first_d; int32_t* first_i;        // scratch: (P, n1_max)
    float* sec_d; int32_t* sec_i;            // scratch: (P, n1_max)
    float* back_d; int32_t* back_i;          // scratch: (P, n2_max)
};

// false: the row is out of range, or image 1 of the pair is empty - nothing to do either way (d_count was cleared)
__device__ __forceinline__ bool ratio_many_row(const RatioMany& g, int p, AffPairRow& r) {
    return aff_pair_row(g.pairs, p, g.rows1, g.rows2, g.n1_max, g.n2_max, r) && r.n1 > 0;
}

// grid (cdiv(rows_max, 64), n_chunks, P), rows = image 1 or, SWAP, image 2 (the backward pass: a pair without rows in image 2 has none).
// out_d / out_i: (P, rows_max, n_chunks, CAP).
template <int CAP, bool FGINN, bool SWAP>
__global__ __launch_bounds__(256) void ratio_many_tile_kernel(RatioMany g, float r2, int tpc, float* __restrict__ out_d, int32_t* __restrict__ out_i) {
    static_assert(!(FGINN && SWAP), "the backward pass has no geometry");
    const int p = blockIdx.z;
    AffPairRow r;
    if (!ratio_many_row(g, p, r)) return;
    if (SWAP && r.n2 == 0) return;
    const float* d1 = g.desc1 + 128 * (size_t)r.row1;
    const float* d2 = g.desc2 + 128 * (size_t)r.row2;
    const size_t o1 = (size_t)p * g.n1_max, o2 = (size_t)p * g.n2_max;
    const size_t o = (SWAP ? o2 : o1) * gridDim.y * CAP;
    if constexpr (SWAP)
        ratio_tile_body<CAP, false>(d2, r.n2, d1, r.n1, g.b_sq + o2, g.a_sq + o1, nullptr, nullptr, r2, tpc, out_d + o, out_i + o, blockIdx.x, blockIdx.y,
                                    gridDim.y);
    else
        ratio_tile_body<CAP, FGINN>(d1, r.n1, d2, r.n2, g.a_sq + o1, g.b_sq + o2, FGINN ? g.lafs2 + 6 * (size_t)r.row2 : nullptr,
                                    FGINN ? g.first_i + o1 : nullptr, r2, tpc, out_d + o, out_i + o, blockIdx.x, blockIdx.y, gridDim.y);
}

// grid (P).  dist / idx: (P, n1_max, 2); tent (P, n1_max, 2); count (P)
template <bool PACK>
__global__ __launch_bounds__(1024) void ratio_many_select_kernel(RatioMany g, float* __restrict__ dist, int32_t* __restrict__ idx, int mutual, float thr,
                                                                 float max_dist, int32_t* __restrict__ tent, int32_t* __restrict__ count) {
    const int p = blockIdx.x;
    AffPairRow r;
    if (!ratio_many_row(g, p, r)) return;
    const size_t o = (size_t)p * g.n1_max;
    ratio_select_body<PACK>(g.first_d + o, g.first_i + o, g.sec_d + o, g.sec_i + o, dist + 2 * o, idx + 2 * o,
                            mutual ? g.back_i + (size_t)p * g.n2_max : (const int32_t*)nullptr, r.n1, thr, max_dist, tent + 2 * o, count + p);
}

// scratch: the single-pair head per pair, array by array (P, n1_max) / (P, n2_max), then the partial lists of the larger of
// (P, n1_max, chunks, 2) and (P, n2_max, chunks, 1)
extern "C" size_t affnet_match_ratio_many_scratch_bytes(int n_pairs, int n1_max, int n2_max, int n_chunks) {
    const size_t P = n_pairs > 0 ? (size_t)n_pairs : 0, a = n1_max > 0 ? (size_t)n1_max : 0, b = n2_max > 0 ? (size_t)n2_max : 0;
    return P * (ratio_head_bytes(a, b) + ratio_part_slots(a, b, n_chunks) * (sizeof(float) + sizeof(int32_t))) + 64;
}

extern "C" int affnet_match_ratio_many(affnet_ctx* ctx, const float* d_desc1, int rows1, const float* d_desc2, int rows2, int dim, const float* d_lafs2,
                                       const int32_t* d_pairs, int n_pairs, int n1_max, int n2_max, float radius, float snn_threshold, float max_dist,
                                       int flags, int n_chunks, float* d_dist, int32_t* d_idx, int32_t* d_tent, int32_t* d_count, void* d_scratch,
                                       void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_desc1 || !d_desc2 || !d_pairs || !d_dist || !d_idx || !d_tent || !d_count || !d_scratch || rows1 < 0 || rows2 < 0 || n_pairs < 0 ||
        n1_max < 0 || n2_max < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "match_ratio_many: bad argument");
    { int rc = ratio_args_check(ctx, "match_ratio_many", dim, d_lafs2, radius, max_dist, flags, n_chunks, d_scratch); if (rc) return rc; }
    if (n_pairs > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "match_ratio_many: %d pairs (at most 65535 per call)", n_pairs);
    if (n_pairs == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)n_pairs, a = (size_t)n1_max, b = (size_t)n2_max;
    { int zrc = aff_zero_async(ctx, d_count, P * sizeof(int32_t), st); if (zrc) return zrc; }
    if (n1_max == 0) return AFFNET_OK;               // image 1 of every pair is empty, or the pair is out of range
    const bool mutual = (flags & AFFNET_RATIO_MUTUAL) != 0, fginn = radius >= 0.0f;
    RatioMany g;
    g.desc1 = d_desc1; g.rows1 = rows1; g.desc2 = d_desc2; g.rows2 = rows2; g.lafs2 = d_lafs2; g.pairs = d_pairs;
    g.n1_max = n1_max; g.n2_max = n2_max;
    g.a_sq = (float*)d_scratch;
    g.first_d = g.a_sq + P * a;
    g.first_i = (int32_t*)(g.first_d + P * a);
    g.sec_d = (float*)(g.first_i + P * a);
    g.sec_i = (int32_t*)(g.sec_d + P * a);
    g.b_sq = (float*)(g.sec_i + P * a);
    g.back_d = g.b_sq + P * b;
    g.back_i = (int32_t*)(g.back_d + P * b);
    const int ncf = ratio_chunks(ctx, n1_max, n2_max, n_chunks, n_pairs), ncb = ratio_chunks(ctx, n2_max, n1_max, n_chunks, n_pairs);
    const size_t fwd = P * a * ncf * 2, bwd = P * b * ncb;
    float* part_d = (float*)((char*)d_scratch + P * ratio_head_bytes(a, b));
    int32_t* part_i = (int32_t*)(part_d + (fwd > bwd ? fwd : bwd));
    const float r2 = radius * radius;
    const unsigned gp = (unsigned)n_pairs;
    const int n1 = n1_max, n2 = n2_max;
    const dim3 gf(aff_cdiv(n1, 64), ncf, gp);
    const int tpcf = aff_cdiv(aff_cdiv(n2, 16), ncf);
    aff_sqnorm_many_launch(st, d_desc1, rows1, d_desc2, rows2, dim, d_pairs, n_pairs, n1_max, n2_max, g.a_sq, g.b_sq);
    if (!fginn) {
        hipLaunchKernelGGL((ratio_many_tile_kernel<2, false, false>), gf, dim3(256), 0, st, g, 0.0f, tpcf, ncf == 1 ? d_dist : part_d, ncf == 1 ? d_idx : part_i);
        if (ncf > 1) aff_knn_merge_pairs_launch(st, part_d, part_i, d_pairs, n_pairs, rows1, rows2, n1, n2, 0, ncf, 2, d_dist, d_idx);
    } else {
        hipLaunchKernelGGL((ratio_many_tile_kernel<1, false, false>), gf, dim3(256), 0, st, g, 0.0f, tpcf, ncf == 1 ? g.first_d : part_d,
                           ncf == 1 ? g.first_i : part_i);
        if (ncf > 1) aff_knn_merge_pairs_launch(st, part_d, part_i, d_pairs, n_pairs, rows1, rows2, n1, n2, 0, ncf, 1, g.first_d, g.first_i);
        hipLaunchKernelGGL((ratio_many_tile_kernel<1, true, false>), gf, dim3(256), 0, st, g, r2, tpcf, ncf == 1 ? g.sec_d : part_d, ncf == 1 ? g.sec_i : part_i);
        if (ncf > 1) aff_knn_merge_pairs_launch(st, part_d, part_i, d_pairs, n_pairs, rows1, rows2, n1, n2, 0, ncf, 1, g.sec_d, g.sec_i);
    }
    if (mutual && n2 > 0) {
        const int tpc = aff_cdiv(aff_cdiv(n1, 16), ncb);
        hipLaunchKernelGGL((ratio_many_tile_kernel<1, false, true>), dim3(aff_cdiv(n2, 64), ncb, gp), dim3(256), 0, st, g, 0.0f, tpc, ncb == 1 ? g.back_d : part_d,
                           ncb == 1 ? g.back_i : part_i);
        if (ncb > 1) aff_knn_merge_pairs_launch(st, part_d, part_i, d_pairs, n_pairs, rows1, rows2, n1, n2, 1, ncb, 1, g.back_d, g.back_i);
    }
    if (fginn) hipLaunchKernelGGL(ratio_many_select_kernel<true>, dim3(gp), dim3(1024), 0, st, g, d_dist, d_idx, mutual ? 1 : 0, snn_threshold, max_dist, d_tent, d_count);
    else hipLaunchKernelGGL(ratio_many_select_kernel<false>, dim3(gp), dim3(1024), 0, st, g, d_dist, d_idx, mutual ? 1 : 0, snn_threshold, max_dist, d_tent, d_count);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
