// Descriptor index, inverted file, for gfx950: a k-means codebook cuts the database rows into cells, the rows are
// stored a second time in cell order, and a query row is compared with the rows of its nprobe nearest cells only (the visual-word index of
// Philbin et al. 2007 with exact distances inside the cells).
//
// The distance is knn.hip's: sqrt(((|a|^2 + |b|^2) - 2 a.b) + 1e-6), a.b by the same chain of 32 v_mfma_f32_16x16x4_f32 over the same K
// order, the squared norms by the same kernel (aff_sqnorm_launch, match.hip), so every distance reported here is the element
// affnet_distance_matrix writes for (query row, ORIGINAL database row), bit for bit.  What is approximate is which rows are looked at, never
// what is reported about one.
//
// Order of candidates, topk.h's: a NaN distance in front of every number, then the smaller distance, then the smaller row.  Inside a
// cell the row is the position in the cell-ordered copy (perm ascends inside every cell, so the order by position IS the order by original
// row); across a row's cells the merge compares original rows.  The order is total and every (query row, cell) pair is processed exactly
// once, so the result does not depend on the order in which the grouping's atomics hand out places.
//
// The lists and their merges are topk.h's, shared with knn.hip and knn_q8.hip, and a row's partial lists are reduced by knn.hip's merge kernel
// (aff_knn_merge_launch).  The tile kernel and the grouping in front of it are this file's own.
#include <math.h>

#include "common.h"
#include "topk.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define IVF_RB 16                     // query rows of one work item: one MFMA row block, shared by the four waves of the workgroup
#define IVF_SCAN_THREADS 1024

// One workgroup per cell, one thread per column: the cell's rows, read through perm in ascending position order, summed into a double;
// centroid = (float)(sum / count).  An empty cell keeps what it has.  No atomics: the bytes repeat run to run.
__global__ __launch_bounds__(128) void ivf_cell_means_kernel(const float* __restrict__ rows, int n, const int32_t* __restrict__ perm,
                                                             const int32_t* __restrict__ cell_start, float* __restrict__ centroids) {
    const int c = blockIdx.x, t = threadIdx.x;
    const int lo = min(max(cell_start[c], 0), n), hi = min(max(cell_start[c + 1], lo), n);
    if (hi <= lo) return;
    double s = 0.0;
    for (int p = lo; p < hi; ++p) {
        const int r = perm[p];
        if ((unsigned)r < (unsigned)n) s += (double)rows[(size_t)r * 128 + t];
    }
    centroids[(size_t)c * 128 + t] = (float)(s / (double)(hi - lo));
}

// ---- grouping: (row -> cells) into (cell -> rows) ----

// partial lists <- (+inf, -1), the cells' counters <- 0
__global__ __launch_bounds__(256) void ivf_init_kernel(float* __restrict__ part_d, int32_t* __restrict__ part_i, long long slots,
                                                       int32_t* __restrict__ count, int n_cells) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < slots) { part_d[e] = INFINITY; part_i[e] = -1; }
    if (e < n_cells) count[e] = 0;
}

__global__ __launch_bounds__(256) void ivf_count_kernel(const int32_t* __restrict__ probes, int n_pairs, int n_cells, int32_t* __restrict__ count) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_pairs) return;
    const int c = probes[e];
    if (c >= 0 && c < n_cells) atomicAdd(&count[c], 1);
}

// One workgroup.  Exclusive scans over the cells of (pairs of the cell, row blocks of the cell): group_start (n_cells + 1), cursor = a
// copy for the scatter, and the table of work items {cell, row block of its group}; meta[0] = the number of items.
__global__ __launch_bounds__(IVF_SCAN_THREADS) void ivf_scan_kernel(const int32_t* __restrict__ count, int n_cells, int32_t* __restrict__ group_start,
                                                                    int32_t* __restrict__ cursor, int2* __restrict__ items, int max_items,
                                                                    int32_t* __restrict__ meta) {
    __shared__ int s_a[IVF_SCAN_THREADS / 64], s_b[IVF_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int base_a = 0, base_b = 0;          // the sums over the cells in front of this round's, equal in every thread
    for (int c0 = 0; c0 < n_cells; c0 += IVF_SCAN_THREADS) {
        const int c = c0 + t;
        const int a = c < n_cells ? count[c] : 0, b = (a + IVF_RB - 1) / IVF_RB;
        int ia = a, ib = b;              // inclusive scans over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
            if (lane >= o) { ia += ua; ib += ub; }
        }
        if (lane == 63) { s_a[wave] = ia; s_b[wave] = ib; }
        __syncthreads();
        int wa = 0, wb = 0, ta = 0, tb = 0;
        for (int w = 0; w < IVF_SCAN_THREADS / 64; ++w) {
            if (w < wave) { wa += s_a[w]; wb += s_b[w]; }
            ta += s_a[w]; tb += s_b[w];
        }
        if (c < n_cells) {
            const int ga = base_a + wa + ia - a, gb = base_b + wb + ib - b;
            group_start[c] = ga;
            cursor[c] = ga;
            for (int j = 0; j < b; ++j)
                if (gb + j < max_items) items[gb + j] = make_int2(c, j);
        }
        base_a += ta; base_b += tb;
        __syncthreads();
    }
    if (t == 0) { group_start[n_cells] = base_a; meta[0] = min(base_b, max_items); }
}

__global__ __launch_bounds__(256) void ivf_scatter_kernel(const int32_t* __restrict__ probes, int n_pairs, int n_cells, int32_t* __restrict__ cursor,
                                                          int32_t* __restrict__ pairs) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_pairs) return;
    const int c = probes[e];
    if (c >= 0 && c < n_cells) pairs[atomicAdd(&cursor[c], 1)] = e;
}

// ---- the tile kernel ----
// One workgroup = one work item = (cell, block of up to 16 pairs of the cell's group).  A pair id is r * nprobe + p: query row r, probe slot p.
// All four waves hold the A fragments of the same 16 gathered query rows (MFMA roles as in knn_tile_kernel: lane (m = l & 15, kq = l >> 4)
// loads row m and holds D[row 4 kq + r][col m]); wave w walks the 16-column tiles w, w + 4, ... of the cell's columns [c_lo, c_hi) of `sorted`,
// tile t at c_lo + 16 t (cells start anywhere), its B fragments loaded straight from memory - no wave shares a tile, so there is nothing to
// stage - with the next tile's loads in flight under the MFMAs.  A lane keeps four lists (one per row) over its columns; per wave the 16
// column lanes of a row are merged, the four waves' lists meet in LDS, and the first k go to the pair's partial list with perm applied.
// A workgroup past the last item, or whose cell is empty, returns in front of the first barrier.
template <int CAP>
__global__ __launch_bounds__(256) void ivf_tile_kernel(const float* __restrict__ q, const float* __restrict__ q_sq, int n1,
                                                       const float* __restrict__ sorted, const float* __restrict__ sorted_sq,
                                                       const int32_t* __restrict__ perm, int n2, const int32_t* __restrict__ cell_start,
                                                       const int32_t* __restrict__ group_start, const int32_t* __restrict__ pairs,
                                                       const int2* __restrict__ items, const int32_t* __restrict__ meta, int nprobe, int k,
                                                       int skip_lo, int skip_hi, float* __restrict__ part_d, int32_t* __restrict__ part_i) {
    constexpr int NG = 8;          // 128 / 16
    __shared__ float s_d[4][IVF_RB][CAP];
    __shared__ int s_i[4][IVF_RB][CAP];
    if ((int)blockIdx.x >= meta[0]) return;
    const int2 item = items[blockIdx.x];
    const int c_lo = min(max(cell_start[item.x], 0), n2), c_hi = min(max(cell_start[item.x + 1], c_lo), n2);
    if (c_hi <= c_lo) return;
    const int g0 = group_start[item.x] + IVF_RB * item.y;
    const int cnt = min(group_start[item.x + 1] - g0, IVF_RB);          // >= 1 by the construction of the items
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 15, kq = lane >> 4;
    const int tiles = (c_hi - c_lo + 15) >> 4;

    f32x4 fa[NG];
    {
        const int r = min(max(pairs[g0 + min(m, cnt - 1)] / nprobe, 0), n1 - 1);
#pragma unroll
        for (int g = 0; g < NG; ++g) fa[g] = *reinterpret_cast<const f32x4*>(&q[(size_t)r * 128 + 16 * g + 4 * kq]);
    }
    float asq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) asq[r] = q_sq[min(max(pairs[g0 + min(4 * kq + r, cnt - 1)] / nprobe, 0), n1 - 1)];
    TopkList<float, CAP> L[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) L[r].clear();

    if (wave < tiles) {          // uniform over the wave; no barrier inside
        f32x4 fb[NG], fn[NG];
        {
            const int cc = min(c_lo + 16 * wave + m, c_hi - 1);
#pragma unroll
            for (int g = 0; g < NG; ++g) fb[g] = *reinterpret_cast<const f32x4*>(&sorted[(size_t)cc * 128 + 16 * g + 4 * kq]);
        }
        for (int t = wave; t < tiles; t += 4) {
            const int col = c_lo + 16 * t + m;
            const int cc = min(col, c_hi - 1);
            // in front of the MFMAs, and no branch between the last MFMA and the accumulator reads (knn.hip, NOTES.md): the next tile's
            // columns are clamped, not predicated (past the wave's last tile they re-read the cell's last row)
            const int cn = min(col + 64, c_hi - 1);
#pragma unroll
            for (int g = 0; g < NG; ++g) fn[g] = *reinterpret_cast<const f32x4*>(&sorted[(size_t)cn * 128 + 16 * g + 4 * kq]);
            const float bsq = sorted_sq[cc];
            const int orig = perm[cc];
            const bool cand = col < c_hi && !(orig >= skip_lo && orig < skip_hi);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[g][j], fb[g][j], acc, 0, 0, 0);
            float d[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = sqrtf(((asq[r] + bsq) - 2.0f * acc[r]) + 1e-6f);      // Losses.py:12-13
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (cand && !(d[r] > L[r].d[CAP - 1])) L[r].insert(d[r], col);
#pragma unroll
            for (int g = 0; g < NG; ++g) fb[g] = fn[g];
        }
    }
    // per wave: the 16 column lanes of a row -> the wave's first k of that row, into LDS (slots behind k are never read)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
            if (j < k) {          // uniform
                float bd;
                int bi;
                topk_lanes_next<16>(L[r], bd, bi);
                if (m == 0) { s_d[wave][4 * kq + r][j] = bd; s_i[wave][4 * kq + r][j] = bi; }
            }
        }
    }
    __syncthreads();
    // wave w merges rows 4 w .. 4 w + 3: lane e < 4 k holds slot e % k of wave e / k
    for (int rr = 0; rr < 4; ++rr) {
        const int row = 4 * wave + rr;
        if (row >= cnt) break;          // uniform over the wave, no barrier behind
        TopkList<float, CAP> M;
        M.clear();
        if (lane < 4 * k) {
            const int ci = s_i[lane / k][row][lane % k];
            if (ci != TOPK_EMPTY) M.insert(s_d[lane / k][row][lane % k], ci);
        }
        const size_t o = (size_t)pairs[g0 + row] * k;
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
            if (j < k) {          // uniform
                float bd;
                int bi;
                topk_lanes_next<64>(M, bd, bi);
                if (lane == 0) { part_d[o + j] = bd; part_i[o + j] = bi == TOPK_EMPTY ? -1 : perm[bi]; }
            }
        }
    }
}

// ---- host ----

extern "C" int affnet_ivf_sqnorm(affnet_ctx* ctx, const float* d_x, int n, int dim, float* d_sq, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_x || !d_sq || n < 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_sqnorm: bad argument");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_sqnorm: descriptor length %d (only 128 is built)", dim);
    if (n == 0) return AFFNET_OK;
    aff_sqnorm_launch((hipStream_t)stream, d_x, n, dim, d_sq);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

extern "C" int affnet_ivf_cell_means(affnet_ctx* ctx, const float* d_rows, int n, int dim, const int32_t* d_perm, const int32_t* d_cell_start,
                                     int n_cells, float* d_centroids, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_rows || !d_perm || !d_cell_start || !d_centroids || n < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_cell_means: bad argument");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_cell_means: descriptor length %d (only 128 is built)", dim);
    if (n_cells < 1) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_cell_means: n_cells = %d", n_cells);
    if (n == 0) return AFFNET_OK;
    hipLaunchKernelGGL(ivf_cell_means_kernel, dim3(n_cells), dim3(128), 0, (hipStream_t)stream, d_rows, n, d_perm, d_cell_start, d_centroids);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// The coarse step's column chunks: affnet_knn's own choice for a 256-CU part, so that the scratch size needs no context.
static int ivf_coarse_chunks(int n1, int n_cells) { return affnet_knn_chunks(nullptr, n1, n_cells); }
// The most it chooses for any n1 (one row block), which is what the scratch is sized for: the size then grows with every argument.
static int ivf_coarse_chunks_most(int n_cells) { return affnet_knn_chunks(nullptr, 1, n_cells); }

// work items of a search: every cell's group cut into blocks of IVF_RB pairs
static long long ivf_max_items(long long n_pairs, long long n_cells) {
    return (n_pairs + IVF_RB - 1) / IVF_RB + (n_cells < n_pairs ? n_cells : n_pairs);
}

// scratch: [coarse knn scratch] [q_sq n1] [coarse dist n1 * nprobe] [probes n1 * nprobe] [count n_cells] [group_start n_cells + 1]
// [cursor n_cells] [meta 4] [pairs n1 * nprobe] [items 2 * max_items] [partial dist n1 * nprobe * k] [partial rows n1 * nprobe * k]
struct IvfLayout {
    size_t coarse, q_sq, cdist, probes, count, group_start, cursor, meta, pairs, items, part_d, part_i, total;
};

static IvfLayout ivf_layout(size_t n1, size_t n_cells, size_t nprobe, size_t k) {
    IvfLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += aff_align(bytes, 16); return at; };
    const size_t np = n1 * nprobe;
    L.coarse = take(affnet_knn_scratch_bytes((int)n1, (int)n_cells, (int)nprobe, ivf_coarse_chunks_most((int)n_cells)));
    L.q_sq = take(n1 * 4);
    L.cdist = take(np * 4);
    L.probes = take(np * 4);
    L.count = take(n_cells * 4);
    L.group_start = take((n_cells + 1) * 4);
    L.cursor = take(n_cells * 4);
    L.meta = take(16);
    L.pairs = take(np * 4);
    L.items = take((size_t)ivf_max_items((long long)np, (long long)n_cells) * 8);
    L.part_d = take(np * k * 4);
    L.part_i = take(np * k * 4);
    L.total = o + 64;
    return L;
}

extern "C" size_t affnet_ivf_scratch_bytes(int n1, int n_cells, int nprobe, int k) {
    return ivf_layout(n1 > 0 ? (size_t)n1 : 0, n_cells > 0 ? (size_t)n_cells : 0, nprobe > 0 ? (size_t)nprobe : 0, k > 0 ? (size_t)k : 0).total;
}

extern "C" int affnet_ivf_search(affnet_ctx* ctx, const float* d_q, int n1, const float* d_sorted, const float* d_sorted_sq, const int32_t* d_perm,
                                 int n2, const int32_t* d_cell_start, const float* d_centroids, int n_cells, int dim, int k, int nprobe,
                                 int skip_row, int skip_n, float* d_dist, int32_t* d_idx, int32_t* d_probes, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_q || !d_sorted || !d_sorted_sq || !d_perm || !d_cell_start || !d_centroids || !d_dist || !d_idx || !d_scratch || n1 < 0 ||
        n2 < 0 || skip_n < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search: bad argument");
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search: descriptor length %d (only 128 is built)", dim);
    if (k < 1 || k > AFFNET_KNN_MAX_K) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search: k = %d (1..%d)", k, AFFNET_KNN_MAX_K);
    if (nprobe < 1 || nprobe > AFFNET_IVF_MAX_PROBE)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search: nprobe = %d (1..%d)", nprobe, AFFNET_IVF_MAX_PROBE);
    if (n_cells < 1) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search: n_cells = %d", n_cells);
    if ((long long)n1 * nprobe * k > 0x7fffffffLL) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search: n1 * nprobe * k = %lld (at most 2^31 - 1)", (long long)n1 * nprobe * k);
    if (n1 == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const IvfLayout L = ivf_layout((size_t)n1, (size_t)n_cells, (size_t)nprobe, (size_t)k);
    char* s = (char*)d_scratch;
    float* q_sq = (float*)(s + L.q_sq);
    float* cdist = (float*)(s + L.cdist);
    int32_t* probes = d_probes ? d_probes : (int32_t*)(s + L.probes);
    int32_t* count = (int32_t*)(s + L.count);
    int32_t* group_start = (int32_t*)(s + L.group_start);
    int32_t* cursor = (int32_t*)(s + L.cursor);
    int32_t* meta = (int32_t*)(s + L.meta);
    int32_t* pairs = (int32_t*)(s + L.pairs);
    int2* items = (int2*)(s + L.items);
    // one probe: a row's only partial list is its result
    float* part_d = nprobe > 1 ? (float*)(s + L.part_d) : d_dist;
    int32_t* part_i = nprobe > 1 ? (int32_t*)(s + L.part_i) : d_idx;
    const int n_pairs = n1 * nprobe;
    const long long slots = (long long)n_pairs * k;
    const int max_items = (int)ivf_max_items(n_pairs, n_cells);
    const AffSkip skip = aff_skip_range(skip_row, skip_n, n2);

    const long long init_n = slots > n_cells ? slots : n_cells;
    hipLaunchKernelGGL(ivf_init_kernel, dim3((unsigned)((init_n + 255) / 256)), dim3(256), 0, st, part_d, part_i, slots, count, n_cells);
    aff_sqnorm_launch(st, d_q, n1, dim, q_sq);
    AFF_LAUNCH_CHECK(ctx);
    {
        const int rc = affnet_knn(ctx, d_q, n1, d_centroids, n_cells, dim, nprobe, 0, 0, ivf_coarse_chunks(n1, n_cells), cdist, probes, s + L.coarse, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ivf_count_kernel, dim3(aff_cdiv(n_pairs, 256)), dim3(256), 0, st, (const int32_t*)probes, n_pairs, n_cells, count);
    hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), dim3(IVF_SCAN_THREADS), 0, st, (const int32_t*)count, n_cells, group_start, cursor, items, max_items, meta);
    hipLaunchKernelGGL(ivf_scatter_kernel, dim3(aff_cdiv(n_pairs, 256)), dim3(256), 0, st, (const int32_t*)probes, n_pairs, n_cells, cursor, pairs);
    aff_topk_dispatch(k, [&](auto cap) {
        hipLaunchKernelGGL((ivf_tile_kernel<decltype(cap)::value>), dim3(max_items), dim3(256), 0, st, d_q, (const float*)q_sq, n1, d_sorted, d_sorted_sq,
                           d_perm, n2, d_cell_start, (const int32_t*)group_start, (const int32_t*)pairs, (const int2*)items, (const int32_t*)meta, nprobe,
                           k, skip.lo, skip.hi, part_d, part_i);
    });
    if (nprobe > 1) aff_knn_merge_launch(st, part_d, part_i, n1, nprobe, k, d_dist, d_idx);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
