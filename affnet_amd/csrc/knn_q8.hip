// Descriptor index on int8 descriptors for gfx950: the quantiser of 128-D descriptors and the exact integer k nearest
// neighbour search over them on v_mfma_i32_16x16x64_i8.  The shortlist (affnet_knn_vote, knn.hip, reads these lists unchanged) needs ranks and a
// ratio gate only; the exact fp32 matcher and the spatial verification still decide what is reported about a pair.
//
// Quantiser, in fp32: q = clamp(rintf(x * scale), -127, 127), one multiply, round half to even, NaN -> 0, +-inf -> +-127; sq = sum q^2 in int32.
// Distance: d2 = (qsq[r] + dbsq[c]) - 2 dot(q[r], db[c]), all int32 and exact: 0 <= d2 <= 128 * 254^2 = 8 258 048 < 2^24, so (float)d2 is exact
// too and the reported distance sqrtf((float)d2) / scale is two correctly rounded fp32 operations.
// Order of candidates: the smaller d2, then the smaller database row - topk.h's order for an int distance, where there is no NaN.  The lists and
// their merges are topk.h's, shared with knn.hip and ivf.hip; an unfilled slot is written out as (INT32_MAX, +inf, -1).
//
// The tile loop is this file's own, knn.hip's restated for the integer instruction (A fragments in registers, the database staged once per workgroup
// through two skewed LDS buffers, the next step's load in flight under the MFMAs, per-lane sorted lists in registers, partial lists per chunk + merge).
// What differs: one MFMA covers K = 64, so a 16 x 16 tile of dot products is 2 MFMAs instead of 32 and the matrix pipe is no longer the bound;
// the staged bytes per workgroup are.  So a step stages 32 columns (4 KB, one 16-byte load per thread) and a wave owns RF fragments of 16
// query rows (8 VGPRs each): 256 rows per workgroup where the lists are short (k <= 2), 128 where they are long (descriptor index, int8).
#include <math.h>

#include "common.h"
#include "topk.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));

#define Q8_DIM 128                    // bytes per row
#define Q8_BS (Q8_DIM + 16)           // bytes per staged column: the 16-byte skew spreads the columns over the banks
#define Q8_STEP 32                    // database columns staged per step = two 16-column MFMA tiles
#define Q8_ROWS_MAX 256               // the larger of the two row blocks (k <= 2): the fewest row blocks, so the most chunks any k takes
#define Q8_WG_PER_CU 2                // the chunk choice: workgroups per CU the grid aims at = what every instantiation keeps resident
#define Q8_MIN_STEPS 2                // the chunk choice: no chunk below this many 32-column steps (descriptor index, int8: the measured floor)
#define Q8_MAX_CHUNKS 1024            // affnet_knn_q8_chunks never chooses more; the size affnet_knn_q8_scratch_bytes assumes for n_chunks = 0

// ---- quantiser ----

__device__ __forceinline__ int q8_quant(float x, float scale) {
    const float v = x * scale;
    return v != v ? 0 : (int)fminf(fmaxf(rintf(v), -127.0f), 127.0f);
}

// 32 lanes per row, 4 elements per lane: grid cdiv(n, 8) x 256 threads.  Rows behind n are clamped for the load and store nothing.
__global__ __launch_bounds__(256) void q8_quantize_kernel(const float* __restrict__ x, int n, float scale, int8_t* __restrict__ q, int32_t* __restrict__ sq) {
    const int row = blockIdx.x * 8 + ((int)threadIdx.x >> 5), part = threadIdx.x & 31;
    const int r = min(row, n - 1);
    const float4 v = *reinterpret_cast<const float4*>(&x[(size_t)r * Q8_DIM + 4 * part]);
    const int a = q8_quant(v.x, scale), b = q8_quant(v.y, scale), c = q8_quant(v.z, scale), d = q8_quant(v.w, scale);
    int s = a * a + b * b + c * c + d * d;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (row < n) {
        *reinterpret_cast<int32_t*>(&q[(size_t)row * Q8_DIM + 4 * part]) = (a & 255) | ((b & 255) << 8) | ((c & 255) << 16) | ((d & 255) << 24);
        if (part == 0) sq[row] = s;
    }
}

extern "C" int affnet_quantize_desc(affnet_ctx* ctx, const float* d_desc, int n, int dim, float scale, int8_t* d_q, int32_t* d_sq, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_desc || !d_q || !d_sq || n < 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "quantize_desc: bad argument");
    if (dim != Q8_DIM) return aff_fail(ctx, AFFNET_ERR_INVALID, "quantize_desc: descriptor length %d (only 128 is built)", dim);
    if (!(scale > 0.0f) || !isfinite(scale)) return aff_fail(ctx, AFFNET_ERR_INVALID, "quantize_desc: scale = %g (finite, > 0)", (double)scale);
    if (n == 0) return AFFNET_OK;
    hipLaunchKernelGGL(q8_quantize_kernel, dim3(aff_cdiv(n, 8)), dim3(256), 0, (hipStream_t)stream, d_desc, n, scale, d_q, d_sq);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// ---- search ----

// The first k of the union of the lists of W lanes: lane `writer` of the group stores round j at slot j, an unfilled slot as (INT32_MAX, +inf, -1).
// out_f: the float distance, or NULL (partial lists).
template <int W, int CAP>
__device__ __forceinline__ void q8_lanes_store(TopkList<int, CAP>& L, int k, bool writer, float scale, int32_t* __restrict__ out_d2,
                                               float* __restrict__ out_f, int32_t* __restrict__ out_i) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        if (j < k) {        // uniform
            int bd, bi;
            topk_lanes_next<W>(L, bd, bi);
            if (writer) {
                out_d2[j] = bd;
                out_i[j] = bi == TOPK_EMPTY ? -1 : bi;
                if (out_f) out_f[j] = bi == TOPK_EMPTY ? INFINITY : sqrtf((float)bd) / scale;
            }
        }
    }
}

// grid (cdiv(n1, 64 RF), n_chunks).  Workgroup = 4 wavefronts; wave w owns the RF fragments of 16 rows at 16 RF w of the workgroup's 64 RF rows
// and walks the 32-column steps [chunk * spc, (chunk + 1) * spc) of `b`.  MFMA roles: A = query rows, B = database columns; lane (m = l & 15,
// kq = l >> 4) gives bytes [16 kq, 16 kq + 16) of row / column m to the first MFMA and [64 + 16 kq, ...) to the second - the same k on both
// sides, which is all a dot product asks of the operand map.  Result layout as in knn.hip: the lane holds D[row 4 kq + r][col m], r = 0..3, so it
// keeps four lists per fragment over the columns = m mod 16 of the chunk, visited in ascending order; the 16 column lanes of a row are merged once,
// at the end of the chunk.  Columns skip_lo <= c < skip_hi are no candidates.
// out_*: (n1, n_chunks, k) - the result itself when there is one chunk (out_f given), else the partial lists q8_merge_kernel reduces (out_f NULL).
// A wave whose rows lie behind n1 computes on clamped rows (every wave must reach the barriers) and writes nothing.
template <int CAP, int RF>
__global__ __launch_bounds__(256) void knn_q8_tile_kernel(const int8_t* __restrict__ a, int n1, const int8_t* __restrict__ b, int n2,
                                                          const int32_t* __restrict__ a_sq, const int32_t* __restrict__ b_sq, int k, int skip_lo,
                                                          int skip_hi, int spc, float scale, int32_t* __restrict__ out_d2, float* __restrict__ out_f,
                                                          int32_t* __restrict__ out_i) {
    __shared__ __attribute__((aligned(16))) unsigned char s_b[2 * Q8_STEP * Q8_BS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * (64 * RF) + wave * (16 * RF);
    const int chunk = blockIdx.y, n_chunks = gridDim.y;
    const int steps = (int)(((long long)n2 + Q8_STEP - 1) / Q8_STEP);
    const long long s0l = (long long)chunk * spc;
    const int s0 = s0l < steps ? (int)s0l : steps, s1 = min(steps, s0 + spc);          // uniform over the workgroup
    TopkList<int, CAP> L[RF][4];
#pragma unroll
    for (int f = 0; f < RF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) L[f][r].clear();
    if (s0 < s1) {
        i32x4 fa[RF][2];
        int asq[RF][4], bound[RF][4];          // bound: per row, no candidate behind it can reach the row's k
#pragma unroll
        for (int f = 0; f < RF; ++f) {
            const int r = min(row0 + 16 * f + m, n1 - 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) fa[f][h] = *reinterpret_cast<const i32x4*>(&a[(size_t)r * Q8_DIM + 64 * h + 16 * kq]);
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                asq[f][r4] = a_sq[min(row0 + 16 * f + 4 * kq + r4, n1 - 1)];
                bound[f][r4] = topk_far<int>();
            }
        }
        // step at column c0 -> one register per thread (columns clamped to the last row of b) and the lane's two sums of squares of that step,
        // so that no load of the loop is waited for in the step that issues it; register -> LDS buffer `buf`
        const int scol = (int)threadIdx.x >> 3, spart = threadIdx.x & 7;
        i32x4 pre;
        int nsq[2];
        auto step_fetch = [&](int c0) {
            const int c = (unsigned)(c0 + scol) < (unsigned)n2 ? c0 + scol : n2 - 1;
            pre = *reinterpret_cast<const i32x4*>(&b[(size_t)c * Q8_DIM + 16 * spart]);
#pragma unroll
            for (int j = 0; j < 2; ++j) nsq[j] = b_sq[(unsigned)(c0 + 16 * j + m) < (unsigned)n2 ? c0 + 16 * j + m : n2 - 1];          // (a column behind n2 may have wrapped)
        };
        auto step_store = [&](int buf) { *reinterpret_cast<i32x4*>(&s_b[(buf * Q8_STEP + scol) * Q8_BS + 16 * spart]) = pre; };
        step_fetch(Q8_STEP * s0);
        step_store(0);
        __syncthreads();
        for (int s = s0; s < s1; ++s) {
            const int c0 = Q8_STEP * s;          // <= n2 - 1
            const int buf = (s - s0) & 1;
            const bool more = s + 1 < s1;
            const int bsq[2] = {nsq[0], nsq[1]};
            if (more) step_fetch(c0 + Q8_STEP);
            // in front of the MFMAs, and no branch between the last MFMA and the accumulator reads (the batched matcher's note)
            int col[2];
            bool cand[2];
            i32x4 fb[2][2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                col[j] = c0 + 16 * j + m;
                cand[j] = (unsigned)col[j] < (unsigned)n2 && !(col[j] >= skip_lo && col[j] < skip_hi);
#pragma unroll
                for (int h = 0; h < 2; ++h) fb[j][h] = *reinterpret_cast<const i32x4*>(&s_b[(buf * Q8_STEP + 16 * j + m) * Q8_BS + 64 * h + 16 * kq]);
            }
            i32x4 acc[RF][2];
#pragma unroll
            for (int f = 0; f < RF; ++f)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const i32x4 zero = {0, 0, 0, 0};
                    acc[f][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[f][0], fb[j][0], zero, 0, 0, 0);
                    acc[f][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[f][1], fb[j][1], acc[f][j], 0, 0, 0);
                }
            int d[RF][2][4];
#pragma unroll
            for (int f = 0; f < RF; ++f)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        d[f][j][r] = (asq[f][r] + bsq[j]) - 2 * acc[f][j][r];
                        // pins the accumulator read here, in straight-line code behind the MFMAs: without it the compiler sinks the reads into the
                        // conditional inserts below, behind a branch (the hazard of DESIGN.md's note at the end of the batched-matcher section)
                        asm volatile("" : "+v"(d[f][j][r]));
                    }
            // tile j = 0 in front of j = 1: a lane's columns arrive in ascending order.  The common case is the first comparison, against the row's bound.
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int f = 0; f < RF; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (cand[j] && d[f][j][r] <= bound[f][r] && d[f][j][r] < L[f][r].d[CAP - 1]) L[f][r].insert(d[f][j][r], col[j]);
            // A lane's own last slot is a weak bound (its list covers a sixteenth of the row's columns): after 4, 8, 16, ... steps, and then every
            // 128, the row's k-th candidate over its 16 lanes becomes the bound.  Uniform over the workgroup.
            const int seen = s - s0 + 1;
            if (seen >= 4 && ((seen & (seen - 1)) == 0 || (seen & 127) == 0)) {
#pragma unroll
                for (int f = 0; f < RF; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) bound[f][r] = topk_lanes_kth<16>(L[f][r], k);
            }
            if (more) step_store(buf ^ 1);      // the other buffer was last read one step ago, in front of that step's barrier
            __syncthreads();
        }
    }
#pragma unroll
    for (int f = 0; f < RF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rr = row0 + 16 * f + 4 * kq + r;
            const size_t o = ((size_t)min(rr, n1 - 1) * n_chunks + chunk) * k;
            q8_lanes_store<16>(L[f][r], k, m == 0 && rr < n1, scale, out_d2 + o, out_f ? out_f + o : nullptr, out_i + o);
        }
}

// One wavefront per row: the n_chunks partial lists (n_chunks * k slots, unfilled ones hold -1) -> the row's k neighbours.
template <int CAP>
__global__ __launch_bounds__(256) void knn_q8_merge_kernel(const int32_t* __restrict__ part_d, const int32_t* __restrict__ part_i, int n1, int n_chunks,
                                                           int k, float scale, int32_t* __restrict__ out_d2, float* __restrict__ out_f,
                                                           int32_t* __restrict__ out_i) {
    const int row = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n1) return;      // uniform over the wave
    TopkList<int, CAP> L;
    L.clear();
    const size_t base = (size_t)row * n_chunks * k;
    const long long total = (long long)n_chunks * k;
    for (long long e = lane; e < total; e += 64) {          // the row's partial slots, strided over the lanes; unfilled ones hold row -1
        const int ci = part_i[base + e];
        if (ci >= 0) L.insert(part_d[base + e], ci);
    }
    const size_t o = (size_t)row * k;
    q8_lanes_store<64>(L, k, lane == 0, scale, out_d2 + o, out_f + o, out_i + o);
}

void aff_knn_q8_merge_launch(hipStream_t st, const int32_t* part_d, const int32_t* part_i, int n1, int n_lists, int k, float scale, int32_t* out_d2,
                             float* out_f, int32_t* out_i) {
    aff_topk_dispatch(k, [&](auto cap) {
        hipLaunchKernelGGL((knn_q8_merge_kernel<decltype(cap)::value>), dim3(aff_cdiv(n1, 4)), dim3(256), 0, st, part_d, part_i, n1, n_lists, k, scale, out_d2,
                           out_f, out_i);
    });
}

struct Q8Args {
    const int8_t *q, *db;
    const int32_t *qsq, *dbsq;
    int n1, n2, k, lo, hi, nc, spc;
    float scale;
    int32_t *part_d, *part_i, *dist2, *idx;
    float* dist;
};

template <int CAP, int RF>
static void knn_q8_launch(hipStream_t st, const Q8Args& a) {
    const dim3 grid(aff_cdiv(a.n1, 64 * RF), a.nc);
    if (a.nc == 1) {
        hipLaunchKernelGGL((knn_q8_tile_kernel<CAP, RF>), grid, dim3(256), 0, st, a.q, a.n1, a.db, a.n2, a.qsq, a.dbsq, a.k, a.lo, a.hi, a.spc, a.scale,
                           a.dist2, a.dist, a.idx);
        return;
    }
    hipLaunchKernelGGL((knn_q8_tile_kernel<CAP, RF>), grid, dim3(256), 0, st, a.q, a.n1, a.db, a.n2, a.qsq, a.dbsq, a.k, a.lo, a.hi, a.spc, a.scale,
                       a.part_d, (float*)nullptr, a.part_i);
    aff_knn_q8_merge_launch(st, a.part_d, a.part_i, a.n1, a.nc, a.k, a.scale, a.dist2, a.dist, a.idx);
}

// The chunks of an n1 x n2 search in row blocks of `rows` query rows: one resident round of workgroups, no chunk below the floor of steps.
static int q8_chunks(const affnet_ctx* ctx, int n1, int n2, int rows) {
    return aff_chunk_choice(ctx, n1 > 0 ? aff_cdiv(n1, rows) : 1, n2 > 0 ? ((long long)n2 + Q8_STEP - 1) / Q8_STEP : 0, Q8_WG_PER_CU, Q8_MIN_STEPS,
                            Q8_MAX_CHUNKS);
}

extern "C" int affnet_knn_q8_chunks(const affnet_ctx* ctx, int n1, int n2) { return q8_chunks(ctx, n1, n2, Q8_ROWS_MAX); }

// scratch: partial d2 int32 (n1, n_chunks, k) | partial rows int32 (n1, n_chunks, k)
extern "C" size_t affnet_knn_q8_scratch_bytes(int n1, int n2, int k, int n_chunks) {
    (void)n2;
    const size_t a = n1 > 0 ? (size_t)n1 : 0, kk = k > 0 ? (size_t)k : 0;
    const size_t nc = n_chunks > 0 ? (size_t)n_chunks : (n_chunks == 0 ? (size_t)Q8_MAX_CHUNKS : 0);
    return a * nc * kk * 2 * sizeof(int32_t) + 64;
}

extern "C" int affnet_knn_q8(affnet_ctx* ctx, const int8_t* d_q, const int32_t* d_qsq, int n1, const int8_t* d_db, const int32_t* d_dbsq, int n2, int dim,
                             int k, int skip_row, int skip_n, int n_chunks, float scale, int32_t* d_dist2, float* d_dist, int32_t* d_idx, void* d_scratch,
                             void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_q || !d_qsq || !d_db || !d_dbsq || !d_dist2 || !d_dist || !d_idx || !d_scratch || n1 < 0 || n2 < 0 || skip_n < 0 || n_chunks < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "knn_q8: bad argument");
    if (dim != Q8_DIM) return aff_fail(ctx, AFFNET_ERR_INVALID, "knn_q8: descriptor length %d (only 128 is built)", dim);
    if (k < 1 || k > AFFNET_KNN_MAX_K) return aff_fail(ctx, AFFNET_ERR_INVALID, "knn_q8: k = %d (1..%d)", k, AFFNET_KNN_MAX_K);
    if (n_chunks > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "knn_q8: %d chunks (at most 65535 per call)", n_chunks);
    if (!(scale > 0.0f) || !isfinite(scale)) return aff_fail(ctx, AFFNET_ERR_INVALID, "knn_q8: scale = %g (finite, > 0)", (double)scale);
    if (n1 == 0) return AFFNET_OK;
    Q8Args a;
    a.q = d_q; a.db = d_db; a.qsq = d_qsq; a.dbsq = d_dbsq;
    a.n1 = n1; a.n2 = n2; a.k = k; a.scale = scale;
    a.nc = n_chunks ? n_chunks : q8_chunks(ctx, n1, n2, aff_topk_cap(k) <= 2 ? 256 : 128);          // <= affnet_knn_q8_chunks(ctx, n1, n2)
    const int steps = (int)(((long long)n2 + Q8_STEP - 1) / Q8_STEP);
    a.spc = aff_cdiv(steps, a.nc);
    const AffSkip skip = aff_skip_range(skip_row, skip_n, n2);
    a.lo = skip.lo; a.hi = skip.hi;
    a.part_d = (int32_t*)d_scratch;
    a.part_i = a.part_d + (size_t)n1 * a.nc * k;
    a.dist2 = d_dist2; a.dist = d_dist; a.idx = d_idx;
    hipStream_t st = (hipStream_t)stream;
    aff_topk_dispatch(k, [&](auto cap) {          // 256 query rows per workgroup where the lists are short, 128 where they are long
        constexpr int CAP = decltype(cap)::value;
        knn_q8_launch<CAP, CAP <= 2 ? 4 : 2>(st, a);
    });
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
