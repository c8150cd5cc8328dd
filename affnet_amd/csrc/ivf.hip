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
//
// The same search over int8 rows in the cells (affnet_ivf_search_q8, further down): the coarse step and the grouping are shared, call for call;
// the distance inside the cells is knn_q8.hip's exact integer d2 on v_mfma_i32_16x16x64_i8, the order (d2, original row), the merge
// knn_q8.hip's (aff_knn_q8_merge_launch).
#include <math.h>

#include "common.h"
#include "topk.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

#define IVF_RB 16                     // query rows of one work item: one MFMA row block, shared by the four waves of the workgroup
#define IVF_SCAN_THREADS 1024
#define IVF_Q8_TILES 4                // int8 cells: 16-column tiles of one wave step = 64 columns, 8 KB of loads per wave in flight

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

// partial lists <- (far, -1) with far = +inf (float lists) or INT32_MAX (int lists), the cells' counters <- 0; part_f: the float distances beside
// int lists that are the result themselves (one probe) <- +inf, or NULL
template <typename D>
__global__ __launch_bounds__(256) void ivf_init_kernel(D* __restrict__ part_d, float* __restrict__ part_f, int32_t* __restrict__ part_i, long long slots,
                                                       D far, int32_t* __restrict__ count, int n_cells) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < slots) {
        part_d[e] = far;
        part_i[e] = -1;
        if (part_f) part_f[e] = INFINITY;
    }
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

// ---- the tile kernel over int8 cells ----
// The same work item, the same roles and the same two merges as ivf_tile_kernel; what differs is the distance and the width of a wave's step.
// d2 = (qsq[r] + sorted_sq[c]) - 2 dot(qq[r], sorted_q[c]) in int32 on v_mfma_i32_16x16x64_i8, operand map as in knn_q8_tile_kernel: lane
// (m = l & 15, kq = l >> 4) gives bytes [16 kq, 16 kq + 16) of its row / column to the first MFMA and [64 + 16 kq, ...) to the second, and holds
// D[row 4 kq + r][col m].  A 16-column tile is 2 KB and 2 MFMAs, so wave w walks the steps w, w + 4, ... of IVF_Q8_TILES tiles (64 columns, 8
// dwordx4 loads per lane) of the cell, step s at c_lo + 64 s, with the next step's rows, sums of squares and perm entries loaded in front of the
// MFMAs.  Columns past the cell's end are clamped for the loads (never predicated) and are no candidates.  A lane meets its columns in ascending
// order.  No bound refresh: a cell gives a wave a handful of steps (descriptor index, inverted file, int8).
// part_d / part_i: the pair's partial list, (INT32_MAX, -1) in unfilled slots; part_f: sqrtf((float)d2) / scale beside it when the partial list
// is the result (one probe), else NULL.
template <int CAP>
__global__ __launch_bounds__(256) void ivf_q8_tile_kernel(const int8_t* __restrict__ q, const int32_t* __restrict__ q_sq, int n1,
                                                          const int8_t* __restrict__ sorted, const int32_t* __restrict__ sorted_sq,
                                                          const int32_t* __restrict__ perm, int n2, const int32_t* __restrict__ cell_start,
                                                          const int32_t* __restrict__ group_start, const int32_t* __restrict__ pairs,
                                                          const int2* __restrict__ items, const int32_t* __restrict__ meta, int nprobe, int k,
                                                          int skip_lo, int skip_hi, float scale, int32_t* __restrict__ part_d,
                                                          float* __restrict__ part_f, int32_t* __restrict__ part_i) {
    constexpr int NT = IVF_Q8_TILES, STEP = 16 * NT;
    __shared__ int s_d[4][IVF_RB][CAP];
    __shared__ int s_i[4][IVF_RB][CAP];
    if ((int)blockIdx.x >= meta[0]) return;
    const int2 item = items[blockIdx.x];
    const int c_lo = min(max(cell_start[item.x], 0), n2), c_hi = min(max(cell_start[item.x + 1], c_lo), n2);
    if (c_hi <= c_lo) return;
    const int g0 = group_start[item.x] + IVF_RB * item.y;
    const int cnt = min(group_start[item.x + 1] - g0, IVF_RB);          // >= 1 by the construction of the items
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 15, kq = lane >> 4;
    const int steps = (c_hi - c_lo + STEP - 1) / STEP;

    i32x4 fa[2];
    {
        const int r = min(max(pairs[g0 + min(m, cnt - 1)] / nprobe, 0), n1 - 1);
#pragma unroll
        for (int h = 0; h < 2; ++h) fa[h] = *reinterpret_cast<const i32x4*>(&q[(size_t)r * 128 + 64 * h + 16 * kq]);
    }
    int asq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) asq[r] = q_sq[min(max(pairs[g0 + min(4 * kq + r, cnt - 1)] / nprobe, 0), n1 - 1)];
    TopkList<int, CAP> L[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) L[r].clear();

    if (wave < steps) {          // uniform over the wave; no barrier inside
        i32x4 fn[NT][2];
        int nsq[NT], norig[NT];
        // the step at column c0: every tile's rows, sums of squares and original rows, the columns clamped to the cell's last row
        auto step_fetch = [&](int c0) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int cc = c0 + min(16 * j + m, c_hi - 1 - c0);          // c0 <= c_hi - 1; no sum past the cell's end is formed
#pragma unroll
                for (int h = 0; h < 2; ++h) fn[j][h] = *reinterpret_cast<const i32x4*>(&sorted[(size_t)cc * 128 + 64 * h + 16 * kq]);
                nsq[j] = sorted_sq[cc];
                norig[j] = perm[cc];
            }
        };
        step_fetch(c_lo + STEP * wave);
        for (int s = wave; s < steps; s += 4) {
            const int c0 = c_lo + STEP * s;          // <= c_hi - 1
            i32x4 fb[NT][2];
            int bsq[NT], col[NT];
            bool cand[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                fb[j][0] = fn[j][0]; fb[j][1] = fn[j][1];
                bsq[j] = nsq[j];
                col[j] = c0 + min(16 * j + m, c_hi - 1 - c0);          // the column that was loaded
                cand[j] = 16 * j + m < c_hi - c0 && !(norig[j] >= skip_lo && norig[j] < skip_hi);
            }
            // in front of the MFMAs, and no branch between the last MFMA and the accumulator reads (knn_q8.hip): past the wave's last
            // step the clamped columns re-read the cell's last row
            step_fetch(c0 < c_hi - 4 * STEP ? c0 + 4 * STEP : c_hi - 1);
            i32x4 acc[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const i32x4 zero = {0, 0, 0, 0};
                acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[0], fb[j][0], zero, 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[1], fb[j][1], acc[j], 0, 0, 0);
            }
            int d[NT][4];
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    d[j][r] = (asq[r] + bsq[j]) - 2 * acc[j][r];
                    asm volatile("" : "+v"(d[j][r]));          // pins the accumulator reads here, behind the last MFMA (knn_q8_tile_kernel)
                }
            // tile j in front of j + 1: ascending columns, so a candidate that only equals the lane's last slot stands behind it
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (cand[j] && d[j][r] < L[r].d[CAP - 1]) L[r].insert(d[j][r], col[j]);
        }
    }
    // per wave: the 16 column lanes of a row -> the wave's first k of that row, into LDS (slots behind k are never read)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
            if (j < k) {          // uniform
                int bd, bi;
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
        TopkList<int, CAP> M;
        M.clear();
        if (lane < 4 * k) {
            const int ci = s_i[lane / k][row][lane % k];
            if (ci != TOPK_EMPTY) M.insert(s_d[lane / k][row][lane % k], ci);
        }
        const size_t o = (size_t)pairs[g0 + row] * k;
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
            if (j < k) {          // uniform
                int bd, bi;
                topk_lanes_next<64>(M, bd, bi);
                if (lane == 0) {
                    part_d[o + j] = bd;
                    part_i[o + j] = bi == TOPK_EMPTY ? -1 : perm[bi];
                    if (part_f) part_f[o + j] = bi == TOPK_EMPTY ? INFINITY : sqrtf((float)bd) / scale;
                }
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
// (both searches; q_sq is the float one's, the partial distances are float or int32)
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

extern "C" size_t affnet_ivf_q8_scratch_bytes(int n1, int n_cells, int nprobe, int k) {          // the same layout, the partial distances int32
    return affnet_ivf_scratch_bytes(n1, n_cells, nprobe, k);
}

// the argument checks both searches share, behind their own pointer checks; `what` names the entry point in the message
static int ivf_check(affnet_ctx* ctx, const char* what, int n1, int n_cells, int dim, int k, int nprobe) {
    if (dim != 128) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: descriptor length %d (only 128 is built)", what, dim);
    if (k < 1 || k > AFFNET_KNN_MAX_K) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: k = %d (1..%d)", what, k, AFFNET_KNN_MAX_K);
    if (nprobe < 1 || nprobe > AFFNET_IVF_MAX_PROBE)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: nprobe = %d (1..%d)", what, nprobe, AFFNET_IVF_MAX_PROBE);
    if (n_cells < 1) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: n_cells = %d", what, n_cells);
    if ((long long)n1 * nprobe * k > 0x7fffffffLL)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: n1 * nprobe * k = %lld (at most 2^31 - 1)", what, (long long)n1 * nprobe * k);
    return AFFNET_OK;
}

// What the grouping leaves for a tile kernel: the cells' groups of pairs, the work items, and the pairs' partial lists, pre-filled.
template <typename D>
struct IvfGroups {
    const int32_t *group_start, *pairs, *meta;
    const int2* items;
    int max_items;
    D* part_d;            // (n1 * nprobe, k): in the scratch, or with one probe the result itself
    float* part_f;        // int lists that are the result: the float distances beside them, else NULL
    int32_t* part_i;
    char* scratch;
    IvfLayout L;
};

// The part of a search both entry points share, n1 >= 1: partial lists <- (far, -1) and the counters <- 0, the coarse step
// affnet_knn(d_q, d_centroids, k = nprobe) -> probes, the (row, cell) pairs grouped by cell (count, scan, scatter).  out_*: the call's outputs,
// which are the partial lists when there is one probe.
template <typename D>
static int ivf_group(affnet_ctx* ctx, const float* d_q, int n1, const float* d_centroids, int n_cells, int dim, int k, int nprobe, D far, D* out_d,
                     float* out_f, int32_t* out_i, int32_t* d_probes, void* d_scratch, void* stream, IvfGroups<D>* g) {
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)d_scratch;
    const IvfLayout L = ivf_layout((size_t)n1, (size_t)n_cells, (size_t)nprobe, (size_t)k);
    float* cdist = (float*)(s + L.cdist);
    int32_t* probes = d_probes ? d_probes : (int32_t*)(s + L.probes);
    int32_t* count = (int32_t*)(s + L.count);
    int32_t* group_start = (int32_t*)(s + L.group_start);
    int32_t* cursor = (int32_t*)(s + L.cursor);
    int32_t* meta = (int32_t*)(s + L.meta);
    int32_t* pairs = (int32_t*)(s + L.pairs);
    int2* items = (int2*)(s + L.items);
    // one probe: a row's only partial list is its result
    g->part_d = nprobe > 1 ? (D*)(s + L.part_d) : out_d;
    g->part_f = nprobe > 1 ? nullptr : out_f;
    g->part_i = nprobe > 1 ? (int32_t*)(s + L.part_i) : out_i;
    const int n_pairs = n1 * nprobe;
    const long long slots = (long long)n_pairs * k;
    g->max_items = (int)ivf_max_items(n_pairs, n_cells);
    g->group_start = group_start; g->pairs = pairs; g->meta = meta; g->items = items; g->scratch = s; g->L = L;

    const long long init_n = slots > n_cells ? slots : n_cells;
    hipLaunchKernelGGL(ivf_init_kernel<D>, dim3((unsigned)((init_n + 255) / 256)), dim3(256), 0, st, g->part_d, g->part_f, g->part_i, slots, far, count,
                       n_cells);
    AFF_LAUNCH_CHECK(ctx);
    {
        const int rc = affnet_knn(ctx, d_q, n1, d_centroids, n_cells, dim, nprobe, 0, 0, ivf_coarse_chunks(n1, n_cells), cdist, probes, s + L.coarse, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ivf_count_kernel, dim3(aff_cdiv(n_pairs, 256)), dim3(256), 0, st, (const int32_t*)probes, n_pairs, n_cells, count);
    hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), dim3(IVF_SCAN_THREADS), 0, st, (const int32_t*)count, n_cells, group_start, cursor, items, g->max_items, meta);
    hipLaunchKernelGGL(ivf_scatter_kernel, dim3(aff_cdiv(n_pairs, 256)), dim3(256), 0, st, (const int32_t*)probes, n_pairs, n_cells, cursor, pairs);
    return AFFNET_OK;
}

extern "C" int affnet_ivf_search(affnet_ctx* ctx, const float* d_q, int n1, const float* d_sorted, const float* d_sorted_sq, const int32_t* d_perm,
                                 int n2, const int32_t* d_cell_start, const float* d_centroids, int n_cells, int dim, int k, int nprobe,
                                 int skip_row, int skip_n, float* d_dist, int32_t* d_idx, int32_t* d_probes, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_q || !d_sorted || !d_sorted_sq || !d_perm || !d_cell_start || !d_centroids || !d_dist || !d_idx || !d_scratch || n1 < 0 ||
        n2 < 0 || skip_n < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search: bad argument");
    if (const int rc = ivf_check(ctx, "ivf_search", n1, n_cells, dim, k, nprobe)) return rc;
    if (n1 == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const AffSkip skip = aff_skip_range(skip_row, skip_n, n2);
    IvfGroups<float> g;
    if (const int rc = ivf_group<float>(ctx, d_q, n1, d_centroids, n_cells, dim, k, nprobe, INFINITY, d_dist, nullptr, d_idx, d_probes, d_scratch, stream, &g))
        return rc;
    float* q_sq = (float*)(g.scratch + g.L.q_sq);
    aff_sqnorm_launch(st, d_q, n1, dim, q_sq);
    aff_topk_dispatch(k, [&](auto cap) {
        hipLaunchKernelGGL((ivf_tile_kernel<decltype(cap)::value>), dim3(g.max_items), dim3(256), 0, st, d_q, (const float*)q_sq, n1, d_sorted, d_sorted_sq,
                           d_perm, n2, d_cell_start, g.group_start, g.pairs, g.items, g.meta, nprobe, k, skip.lo, skip.hi, g.part_d, g.part_i);
    });
    if (nprobe > 1) aff_knn_merge_launch(st, g.part_d, g.part_i, n1, nprobe, k, d_dist, d_idx);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

extern "C" int affnet_ivf_search_q8(affnet_ctx* ctx, const float* d_q, const int8_t* d_qq, const int32_t* d_qsq, int n1, const int8_t* d_sorted_q,
                                    const int32_t* d_sorted_sq, const int32_t* d_perm, int n2, const int32_t* d_cell_start, const float* d_centroids,
                                    int n_cells, int dim, int k, int nprobe, int skip_row, int skip_n, float scale, int32_t* d_dist2, float* d_dist,
                                    int32_t* d_idx, int32_t* d_probes, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_q || !d_qq || !d_qsq || !d_sorted_q || !d_sorted_sq || !d_perm || !d_cell_start || !d_centroids || !d_dist2 || !d_dist || !d_idx ||
        !d_scratch || n1 < 0 || n2 < 0 || skip_n < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search_q8: bad argument");
    if (const int rc = ivf_check(ctx, "ivf_search_q8", n1, n_cells, dim, k, nprobe)) return rc;
    if (!(scale > 0.0f) || !isfinite(scale)) return aff_fail(ctx, AFFNET_ERR_INVALID, "ivf_search_q8: scale = %g (finite, > 0)", (double)scale);
    if (n1 == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const AffSkip skip = aff_skip_range(skip_row, skip_n, n2);
    IvfGroups<int32_t> g;
    if (const int rc = ivf_group<int32_t>(ctx, d_q, n1, d_centroids, n_cells, dim, k, nprobe, 0x7fffffff, d_dist2, d_dist, d_idx, d_probes, d_scratch, stream, &g))
        return rc;
    aff_topk_dispatch(k, [&](auto cap) {
        hipLaunchKernelGGL((ivf_q8_tile_kernel<decltype(cap)::value>), dim3(g.max_items), dim3(256), 0, st, d_qq, d_qsq, n1, d_sorted_q, d_sorted_sq, d_perm, n2,
                           d_cell_start, g.group_start, g.pairs, g.items, g.meta, nprobe, k, skip.lo, skip.hi, scale, g.part_d, g.part_f, g.part_i);
    });
    if (nprobe > 1) aff_knn_q8_merge_launch(st, g.part_d, g.part_i, n1, nprobe, k, scale, d_dist2, d_dist, d_idx);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
