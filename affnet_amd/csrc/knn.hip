// Descriptor index for gfx950: k nearest neighbours of query descriptors among the concatenated descriptors of many
// images, and one vote per image from them - the shortlist that affnet_match_snn_many / affnet_verify_matches_many (match.hip, spatial.hip) re-rank.
//
// The distance is the matcher's (match.hip, rowmin_dist_body; Losses.py:5-13): sqrt(((|a|^2 + |b|^2) - 2 a.b) + 1e-6), a.b by the same chain
// of v_mfma_f32_16x16x4_f32 over the same K order, the squared norms by the same reduction, so every distance reported here is the element
// affnet_distance_matrix writes for that (row, column), bit for bit.  The tile loop is the matcher's STAGE form restated (A fragments of 16 rows
// per wave in registers, the B tile staged once per workgroup through two skewed LDS buffers, the next tile's loads in flight under the MFMAs);
// what differs is that a workgroup walks only the 16-column tiles of ITS chunk of the database (grid = row blocks x chunks, so that a large
// database fills the part whatever the number of query rows) and keeps up to 8 neighbours per row instead of one.
//
// The order of candidates, the lists and their merges: topk.h, shared with knn_q8.hip and ivf.hip.  The squared norms: match.hip's own kernel
// (aff_sqnorm_launch), so the equality with affnet_distance_matrix rests on one definition.
#include <math.h>

#include "common.h"
#include "topk.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define KNN_BS(DIM) ((DIM) + 4)       // floats per staged column: the 16-byte skew spreads the 16 columns over the banks (match.hip ROWMIN_BS)
#define KNN_WG_PER_CU 3               // affnet_knn_chunks: workgroups per CU the grid aims at (what the k = 8 kernel keeps resident; DESIGN.md, descriptor index)
#define KNN_MIN_TILES 5               // affnet_knn_chunks: no chunk below this many 16-column tiles (descriptor index: the measured floor)
#define KNN_MAX_CHUNKS 1024           // affnet_knn_chunks never chooses more; the size affnet_knn_scratch_bytes assumes for n_chunks = 0

// The first k of the union of the lists of W lanes: lane `writer` of the group stores round j at out[j], an unfilled slot as -1.
template <int W, int CAP>
__device__ __forceinline__ void knn_lanes_store(TopkList<float, CAP>& L, int k, bool writer, float* __restrict__ out_d, int32_t* __restrict__ out_i) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        if (j < k) {        // uniform
            float bd;
            int bi;
            topk_lanes_next<W>(L, bd, bi);
            if (writer) { out_d[j] = bd; out_i[j] = bi == TOPK_EMPTY ? -1 : bi; }
        }
    }
}

// grid (cdiv(n1, 64), n_chunks).  Workgroup = 4 wavefronts = 64 rows of `a`; wave w owns rows 16w..16w+15 and walks the tiles
// [chunk * tpc, (chunk + 1) * tpc) of `b`.  MFMA roles and result layout as in rowmin_dist_body: lane (n = l & 15, g = l >> 4) holds
// D[row 4 g + r][col n], r = 0..3, so a lane keeps four lists (one per row) over the columns = n mod 16 of the chunk; the 16 column lanes of a
// row are merged once, at the end of the chunk.  Columns skip_lo <= c < skip_hi are no candidates.
// out_d / out_i: (n1, n_chunks, k) - the result itself when there is one chunk, else the partial lists knn_merge_kernel reduces.
// A wave whose 16 rows lie behind n1 computes on clamped rows (every wave must reach the barriers) and writes nothing.
template <int DIM, int CAP>
__global__ __launch_bounds__(256) void knn_tile_kernel(const float* __restrict__ a, int n1, const float* __restrict__ b, int n2,
                                                       const float* __restrict__ a_sq, const float* __restrict__ b_sq, int k, int skip_lo,
                                                       int skip_hi, int tpc, float* __restrict__ out_d, int32_t* __restrict__ out_i) {
    constexpr int NG = DIM / 16;
    constexpr int BS = KNN_BS(DIM), Q = DIM / 4, NPRE = 16 * Q / 256;      // float4 per column, float4 per thread and tile
    static_assert((16 * Q) % 256 == 0, "the staged tile is loaded by 256 threads in whole rounds");
    __shared__ __attribute__((aligned(16))) float s_b[2 * 16 * BS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * 64 + wave * 16;
    const int chunk = blockIdx.y, n_chunks = gridDim.y;
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
#pragma unroll
        for (int r = 0; r < 4; ++r) asq[r] = a_sq[min(row0 + 4 * kq + r, n1 - 1)];
        float bound[4] = {INFINITY, INFINITY, INFINITY, INFINITY};      // per row: no candidate behind it can reach the row's k
        f32x4 pre[NPRE];
        // tile at column c0 -> registers (columns clamped to the last row of b); registers -> LDS buffer `buf`
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
            const bool cand = col < n2 && !(col >= skip_lo && col < skip_hi);
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
                // the common case is the first comparison, against the row's bound (a NaN on either side goes on to the full test)
                if (cand && !(d[r] > bound[r]) && !(d[r] > L[r].d[CAP - 1])) L[r].insert(d[r], col);
            }
            // A lane's own last slot is a weak bound (its list covers a sixteenth of the row's columns): after 8, 16, 32, ... tiles, and then every
            // 256, the row's k-th candidate over its 16 lanes becomes the bound.  Uniform over the workgroup.
            const int seen = t - t0 + 1;
            if (seen >= 8 && ((seen & (seen - 1)) == 0 || (seen & 255) == 0)) {
#pragma unroll
                for (int r = 0; r < 4; ++r) bound[r] = topk_lanes_kth<16>(L[r], k);
            }
            if (more) tile_store(buf ^ 1);      // the other buffer was last read one tile ago, in front of that tile's barrier
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = min(row0 + 4 * kq + r, n1 - 1);
        const size_t o = ((size_t)row * n_chunks + chunk) * k;
        knn_lanes_store<16>(L[r], k, m == 0 && row0 + 4 * kq + r < n1, out_d + o, out_i + o);
    }
}

// One wavefront per row: the n_lists partial lists of the row (the chunks of a search here, the probed cells of one in ivf.hip) -> its k neighbours.
template <int CAP>
__device__ __forceinline__ void knn_merge_body(const float* __restrict__ part_d, const int32_t* __restrict__ part_i, int n1, int n_lists, int k,
                                               float* __restrict__ out_d, int32_t* __restrict__ out_i, int blk) {
    const int row = blk * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n1) return;      // uniform over the wave
    TopkList<float, CAP> L;
    L.clear();
    const size_t base = (size_t)row * n_lists * k;
    const long long total = (long long)n_lists * k;
    for (long long e = lane; e < total; e += 64) {          // the row's partial slots, strided over the lanes; unfilled ones hold row -1
        const int ci = part_i[base + e];
        if (ci >= 0) L.insert(part_d[base + e], ci);
    }
    knn_lanes_store<64>(L, k, lane == 0, out_d + (size_t)row * k, out_i + (size_t)row * k);
}

template <int CAP>
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part_d, const int32_t* __restrict__ part_i, int n1, int n_lists,
                                                        int k, float* __restrict__ out_d, int32_t* __restrict__ out_i) {
    knn_merge_body<CAP>(part_d, part_i, n1, n_lists, k, out_d, out_i, blockIdx.x);
}

void aff_knn_merge_launch(hipStream_t st, const float* part_d, const int32_t* part_i, int n1, int n_lists, int k, float* out_d, int32_t* out_i) {
    aff_topk_dispatch(k, [&](auto cap) {
        hipLaunchKernelGGL((knn_merge_kernel<decltype(cap)::value>), dim3(aff_cdiv(n1, 4)), dim3(256), 0, st, part_d, part_i, n1, n_lists, k, out_d, out_i);
    });
}

// The same merge for the pairs of a *_many call, grid (rows_max / 4, P): pair p merges the rows of its side `side` (0: n1 rows, pitch n1_max;
// 1: n2 rows, pitch n2_max) of pair-major partial lists (P, pitch, n_lists, k) into pair-major outputs (P, pitch, k).  The table row is tested
// before anything is loaded; a pair out of range or with an empty side 1 (it has no lists on either side) and the rows at or beyond the pair's
// own count are neither read nor written.
template <int CAP>
__global__ __launch_bounds__(256) void knn_merge_pairs_kernel(const float* __restrict__ part_d, const int32_t* __restrict__ part_i,
                                                              const int32_t* __restrict__ pairs, int rows1, int rows2, int n1_max, int n2_max, int side,
                                                              int n_lists, int k, float* __restrict__ out_d, int32_t* __restrict__ out_i) {
    const int p = blockIdx.y;
    AffPairRow r;
    if (!aff_pair_row(pairs, p, rows1, rows2, n1_max, n2_max, r) || r.n1 == 0) return;
    const size_t o = (size_t)p * (side ? n2_max : n1_max);
    knn_merge_body<CAP>(part_d + o * n_lists * k, part_i + o * n_lists * k, side ? r.n2 : r.n1, n_lists, k, out_d + o * k, out_i + o * k, blockIdx.x);
}

void aff_knn_merge_pairs_launch(hipStream_t st, const float* part_d, const int32_t* part_i, const int32_t* pairs, int n_pairs, int rows1, int rows2,
                                int n1_max, int n2_max, int side, int n_lists, int k, float* out_d, int32_t* out_i) {
    const int rows_max = side ? n2_max : n1_max;
    if (n_pairs <= 0 || rows_max <= 0) return;
    aff_topk_dispatch(k, [&](auto cap) {
        hipLaunchKernelGGL((knn_merge_pairs_kernel<decltype(cap)::value>), dim3(aff_cdiv(rows_max, 4), (unsigned)n_pairs), dim3(256), 0, st, part_d, part_i,
                           pairs, rows1, rows2, n1_max, n2_max, side, n_lists, k, out_d, out_i);
    });
}

extern "C" int affnet_knn_chunks(const affnet_ctx* ctx, int n1, int n2) {
    return aff_chunk_choice(ctx, n1 > 0 ? aff_cdiv(n1, 64) : 1, n2 > 0 ? ((long long)n2 + 15) / 16 : 0, KNN_WG_PER_CU, KNN_MIN_TILES, KNN_MAX_CHUNKS);
}

// scratch: a_sq float (n1) | b_sq float (n2) | partial distances float (n1, n_chunks, k) | partial rows int32 (n1, n_chunks, k)
static size_t knn_norm_bytes(size_t n1, size_t n2) { return aff_align((n1 + n2) * sizeof(float), 16); }

extern "C" size_t affnet_knn_scratch_bytes(int n1, int n2, int k, int n_chunks) {
    const size_t a = n1 > 0 ? (size_t)n1 : 0, b = n2 > 0 ? (size_t)n2 : 0, kk = k > 0 ? (size_t)k : 0;
    const size_t nc = n_chunks > 0 ? (size_t)n_chunks : (n_chunks == 0 ? (size_t)KNN_MAX_CHUNKS : 0);
    return knn_norm_bytes(a, b) + a * nc * kk * (sizeof(float) + sizeof(int32_t)) + 64;
}

extern "C" int affnet_knn(affnet_ctx* ctx, const float* d_q, int n1, const float* d_db, int n2, int dim, int k, int skip_row, int skip_n,
                          int n_chunks, float* d_dist, int32_t* d_idx, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_q || !d_db || !d_dist || !d_idx || !d_scratch || n1 < 0 || n2 < 0 || skip_n < 0 || n_chunks < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "knn: bad argument");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "knn: descriptor length %d (only 128 is built)", dim);
    if (k < 1 || k > AFFNET_KNN_MAX_K) return aff_fail(ctx, AFFNET_ERR_INVALID, "knn: k = %d (1..%d)", k, AFFNET_KNN_MAX_K);
    if (n_chunks > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "knn: %d chunks (at most 65535 per call)", n_chunks);
    if (n1 == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const int nc = n_chunks ? n_chunks : affnet_knn_chunks(ctx, n1, n2);
    const int tiles = (int)(((long long)n2 + 15) / 16), tpc = aff_cdiv(tiles, nc);
    const AffSkip skip = aff_skip_range(skip_row, skip_n, n2);
    float* a_sq = (float*)d_scratch;
    float* b_sq = a_sq + n1;
    float* part_d = (float*)((char*)d_scratch + knn_norm_bytes((size_t)n1, (size_t)n2));
    int32_t* part_i = (int32_t*)(part_d + (size_t)n1 * nc * k);
    aff_sqnorm_launch(st, d_q, n1, dim, a_sq);
    aff_sqnorm_launch(st, d_db, n2, dim, b_sq);
    // one chunk: its lists are the result
    float* tile_d = nc == 1 ? d_dist : part_d;
    int32_t* tile_i = nc == 1 ? d_idx : part_i;
    aff_topk_dispatch(k, [&](auto cap) {
        hipLaunchKernelGGL((knn_tile_kernel<128, decltype(cap)::value>), dim3(aff_cdiv(n1, 64), nc), dim3(256), 0, st, d_q, n1, d_db, n2,
                           (const float*)a_sq, (const float*)b_sq, k, skip.lo, skip.hi, tpc, tile_d, tile_i);
    });
    if (nc > 1) aff_knn_merge_launch(st, part_d, part_i, n1, nc, k, d_dist, d_idx);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// One thread per query row.  voted[]: the images this row has voted for, compile-time indices only.
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ dist, const int32_t* __restrict__ idx, int n1, int k, float ratio,
                                                       const int32_t* __restrict__ row_image, int n2, int n_images, int32_t* __restrict__ votes) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n1) return;
    const float bound = ratio * dist[(size_t)r * k + (k - 1)];
    int voted[AFFNET_KNN_MAX_K - 1];
#pragma unroll
    for (int j = 0; j < AFFNET_KNN_MAX_K - 1; ++j) {
        voted[j] = -1;
        if (j < k - 1) {
            const int c = idx[(size_t)r * k + j];
            if (c >= 0 && c < n2) {
                const int img = row_image[c];
                bool ok = img >= 0 && img < n_images && !(dist[(size_t)r * k + j] > bound);
#pragma unroll
                for (int e = 0; e < j; ++e) ok = ok && voted[e] != img;
                if (ok) { voted[j] = img; atomicAdd(&votes[img], 1); }
            }
        }
    }
}

extern "C" int affnet_knn_vote(affnet_ctx* ctx, const float* d_dist, const int32_t* d_idx, int n1, int k, float ratio, const int32_t* d_row_image,
                               int n2, int n_images, int32_t* d_votes, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_dist || !d_idx || !d_row_image || !d_votes || n1 < 0 || n2 < 0 || n_images < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "knn_vote: bad argument");
    if (k < 1 || k > AFFNET_KNN_MAX_K) return aff_fail(ctx, AFFNET_ERR_INVALID, "knn_vote: k = %d (1..%d)", k, AFFNET_KNN_MAX_K);
    hipStream_t st = (hipStream_t)stream;
    if (n_images == 0) return AFFNET_OK;
    { int zrc = aff_zero_async(ctx, d_votes, (size_t)n_images * sizeof(int32_t), st); if (zrc) return zrc; }
    if (n1 == 0 || k == 1) return AFFNET_OK;
    hipLaunchKernelGGL(knn_vote_kernel, dim3(aff_cdiv(n1, 256)), dim3(256), 0, st, d_dist, d_idx, n1, k, ratio, d_row_image, n2, n_images, d_votes);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
