// Spatial verification of tentative matches from their local affine frames, for gfx950 ("f1 verification").
//
// One tentative match of two affine frames fixes a full affine map F2 F1^-1 (the spatial matching of Philbin et al., CVPR 2007), so T
// tentatives give exactly T hypotheses and every one of them is scored against all T matches: a T x T pairwise kernel with K = 2, i.e.
// VALU work, no matrix cores.  The best hypothesis is then refined by a few least-squares refits (homography or affine) on its inliers
// in fp64.  No random number, no data-dependent loop bound, the same answer on every run.
//
//   spv_prep_kernel    per tentative: gather the two frames through `tent`, centres -> pts[t] = (x1, y1, x2, y2), M = L2 L1^-1 -> hyp[t],
//                      counts[t] = 0.  An invalid match (index out of range - tested BEFORE any load - or a non-finite centre) gets NaN
//                      centres, an invalid hypothesis (that, a non-finite entry, or !(|det L1| > 1e-12)) a NaN matrix: every comparison
//                      with a NaN error is false, so neither is ever an inlier / ever has one, without a branch in the pair loop.
//   spv_score_kernel   2-D grid (hypothesis tile SPV_HT) x (match chunk SPV_MC).  One thread = one hypothesis in registers; the chunk's
//                      matches sit in LDS as float4 and every lane reads the same address (one ds_read_b128, a broadcast).  One integer
//                      atomicAdd per thread and chunk: integer sums do not depend on the order of arrival.
//   spv_select_kernel  one workgroup: smallest h with the largest count, -1 when that count is 0.
//   spv_lo_kernel      one workgroup, fp64: local optimisation of the best hypothesis.  Sums over pairs go registers (a fixed stride of
//                      pairs per thread) -> wave butterfly -> LDS -> one thread per sum, in one fixed order; the normal equations are
//                      eliminated by one thread on a matrix held in LDS (a per-thread runtime-indexed array would live in scratch).
//
// The row count comes from a device pointer (what affnet_match_snn writes), rows at or beyond it are neither read nor written.
//
// affnet_verify_matches_many (end of the file) runs the same four stages for P image pairs per launch: spv_many_*_kernel take the pair index from
// the grid, find the pair's segments in a device table and call the bodies of the kernels above.
#include <math.h>

#include "common.h"
#include "spatial_dev.h"

#define SPV_HT 128          // hypotheses per workgroup of the scoring kernel = its workgroup size (AFFNET_VERIFY_TILE)
#define SPV_MC 128          // matches per LDS chunk (AFFNET_VERIFY_CHUNK)
#define SPV_LO_THREADS 256
#define SPV_NSUM 44         // sums of the homography normal equations: 36 of the upper triangle + 8 of the right-hand side

static_assert(SPV_HT == AFFNET_VERIFY_TILE && SPV_MC == AFFNET_VERIFY_CHUNK, "include/affnet_hip.h states the tile sizes");

// The scoring rule, fp32, centre-relative: e = | M (c1_t - c1_h) - (c2_t - c2_h) |^2 <= th^2.  No fused multiply-add (the file is built with
// -ffp-contract=off), so the local optimisation's start mask below is the scoring kernel's inlier set bit for bit.
__device__ __forceinline__ bool spv_inlier(const float4 m, const float4 ph, const float4 pt, float th2) {
    const float dx = pt.x - ph.x, dy = pt.y - ph.y;
    const float u = (m.x * dx + m.y * dy) - (pt.z - ph.z);
    const float v = (m.z * dx + m.w * dy) - (pt.w - ph.w);
    return (u * u + v * v) <= th2;
}

// The *_body functions are the kernels of one image pair; the __global__ kernels, single-pair here and batched at the end of the file (pair index on
// a grid dimension), only choose the pointers and the workgroup indices they run on.
__device__ __forceinline__ void spv_prep_body(const SpvIn& in, float4* __restrict__ pts, float4* __restrict__ hyp, int32_t* __restrict__ counts, int blk) {
    const int t = blk * 256 + threadIdx.x;
    if (t >= spv_rows(in.count, in.t_max)) return;
    const float qn = __builtin_nanf("");
    float4 p = make_float4(qn, qn, qn, qn), m = p;
    float A[6], B[6];
    if (spv_gather(in, t, A, B)) {
        const float a = A[0], b = A[1], x1 = A[2], c = A[3], d = A[4], y1 = A[5];
        const float a2 = B[0], b2 = B[1], x2 = B[2], c2 = B[3], d2 = B[4], y2 = B[5];
        const bool centres = spv_centres_finite(A, B);
        if (centres) p = make_float4(x1, y1, x2, y2);
        const float det = a * d - b * c;
        // M = L2 L1^-1, L1^-1 = [d -b; -c a] / det
        if (centres && spv_shapes_finite(A, B) && fabsf(det) > 1e-12f)
            m = make_float4((a2 * d - b2 * c) / det, (b2 * a - a2 * b) / det, (c2 * d - d2 * c) / det, (d2 * a - c2 * b) / det);
    }
    pts[t] = p; hyp[t] = m; counts[t] = 0;
}

__global__ __launch_bounds__(256) void spv_prep_kernel(SpvIn in, float4* __restrict__ pts, float4* __restrict__ hyp, int32_t* __restrict__ counts) {
    spv_prep_body(in, pts, hyp, counts, blockIdx.x);
}

__device__ __forceinline__ void spv_score_body(const float4* __restrict__ pts, const float4* __restrict__ hyp, const int32_t* __restrict__ count, int t_max,
                                               float th2, int32_t* __restrict__ counts, int blk_h, int blk_t) {
    __shared__ float4 s_pt[SPV_MC];
    const int rows = spv_rows(count, t_max);
    const int h0 = blk_h * SPV_HT, t0 = blk_t * SPV_MC;
    if (h0 >= rows || t0 >= rows) return;                     // uniform over the workgroup
    const int nt = min(SPV_MC, rows - t0);
    for (int k = threadIdx.x; k < nt; k += SPV_HT) s_pt[k] = pts[t0 + k];
    __syncthreads();
    const int h = h0 + threadIdx.x;
    if (h >= rows) return;
    const float4 m = hyp[h], ph = pts[h];
    int c = 0;
    for (int k = 0; k < nt; ++k) c += spv_inlier(m, ph, s_pt[k], th2) ? 1 : 0;
    if (c) atomicAdd(&counts[h], c);
}

__global__ __launch_bounds__(SPV_HT) void spv_score_kernel(const float4* __restrict__ pts, const float4* __restrict__ hyp, const int32_t* __restrict__ count,
                                                           int t_max, float th2, int32_t* __restrict__ counts) {
    spv_score_body(pts, hyp, count, t_max, th2, counts, blockIdx.x, blockIdx.y);
}

// best[0] = smallest h with the largest count, best[1] = that count; {-1, 0} when no hypothesis has an inlier (no valid hypothesis, or no rows)
__device__ __forceinline__ void spv_select_body(const int32_t* __restrict__ counts, const int32_t* __restrict__ count, int t_max, int32_t* __restrict__ best) {
    spv_select_rows(counts, spv_rows(count, t_max), best);
}

__global__ __launch_bounds__(256) void spv_select_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ count, int t_max,
                                                         int32_t* __restrict__ best) {
    spv_select_body(counts, count, t_max, best);
}

// ---- local optimisation ---------------------------------------------------------------------------------------------------------------
struct SpvLo {
    SpvIn in;
    const float4* pts; const float4* hyp;
    const int32_t* best;       // {index, count} of spv_select_kernel
    float th; int model; int lo_iters;
    uint8_t* cur;              // scratch: the current mask
    double* model_out; uint8_t* inlier; int32_t* summary;
};

// Gaussian elimination with partial pivoting of the n x m augmented matrix A (m - n right-hand sides) in LDS, by one thread; the solutions
// replace the right-hand sides.  false: a pivot below `tiny` (or a NaN).
__device__ __forceinline__ bool spv_solve_lds(double* A, int n, int m, double tiny) {
    for (int c = 0; c < n; ++c) {
        int p = c;
        double pv = fabs(A[c * m + c]);
        for (int r = c + 1; r < n; ++r)
            if (fabs(A[r * m + c]) > pv) { pv = fabs(A[r * m + c]); p = r; }
        if (!(pv >= tiny)) return false;
        if (p != c)
            for (int k = c; k < m; ++k) { const double s = A[c * m + k]; A[c * m + k] = A[p * m + k]; A[p * m + k] = s; }
        for (int r = c + 1; r < n; ++r) {
            const double f = A[r * m + c] / A[c * m + c];
            for (int k = c; k < m; ++k) A[r * m + k] -= f * A[c * m + k];
        }
    }
    for (int q = n; q < m; ++q)
        for (int c = n - 1; c >= 0; --c) {
            double x = A[c * m + q];
            for (int k = c + 1; k < n; ++k) x -= A[c * m + k] * A[k * m + q];
            A[c * m + q] = x / A[c * m + c];
        }
    return true;
}

// C = A B, 3 x 3, all in LDS (one thread)
__device__ __forceinline__ void spv_mul3_lds(const double* A, const double* B, double* Cm) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Cm[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

__device__ __forceinline__ void spv_lo_body(const SpvLo& a) {
    __shared__ double s_part[4 * SPV_NSUM], s_sum[SPV_NSUM];
    __shared__ double s_A[8 * 9];
    __shared__ double s_m[4][9];           // 0: candidate model, 1: kept model, 2 / 3: denormalisation factors
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    const int rows = spv_rows(a.in.count, a.in.t_max);
    const int best = a.best[0];
    if (best < 0) {                        // no valid hypothesis (or no rows): identity, empty mask, flag 1
        for (int t = tid; t < rows; t += SPV_LO_THREADS) a.inlier[t] = 0;
        if (tid < 9) a.model_out[tid] = (tid % 4 == 0) ? 1.0 : 0.0;
        if (tid == 0) { a.summary[0] = -1; a.summary[1] = 0; a.summary[2] = 0; a.summary[3] = 1; }
        return;
    }
    // model 0: the affine hypothesis itself, in fp64 from the two frames (their indices passed the guard of spv_prep_kernel: the hypothesis is valid)
    if (tid == 0) {
        const float* A = a.in.lafs1 + 6 * (size_t)a.in.tent[2 * best];
        const float* B = a.in.lafs2 + 6 * (size_t)a.in.tent[2 * best + 1];
        const double la = A[0], lb = A[1], x1 = A[2], lc = A[3], ld = A[4], y1 = A[5];
        const double a2 = B[0], b2 = B[1], x2 = B[2], c2 = B[3], d2 = B[4], y2 = B[5];
        const double det = la * ld - lb * lc;
        const double m00 = (a2 * ld - b2 * lc) / det, m01 = (b2 * la - a2 * lb) / det, m10 = (c2 * ld - d2 * lc) / det, m11 = (d2 * la - c2 * lb) / det;
        double* H = s_m[1];
        H[0] = m00; H[1] = m01; H[2] = x2 - (m00 * x1 + m01 * y1);
        H[3] = m10; H[4] = m11; H[5] = y2 - (m10 * x1 + m11 * y1);
        H[6] = 0.0; H[7] = 0.0; H[8] = 1.0;
        s_stop = 0;
    }
    const float th2f = a.th * a.th;
    const double th2 = (double)a.th * (double)a.th;
    int n_cur, n_best, flags = 0;
    {
        const float4 m = a.hyp[best], ph = a.pts[best];
        double v[1] = {0.0};
        for (int t = tid; t < rows; t += SPV_LO_THREADS) {
            const bool in = spv_inlier(m, ph, a.pts[t], th2f);
            a.cur[t] = in; a.inlier[t] = in;           // thread tid owns rows tid, tid + 256, ... of both masks throughout
            v[0] += in ? 1.0 : 0.0;
        }
        spv_block_sum<1>(v, s_part, s_sum);
        n_cur = n_best = (int)v[0];
    }
    const int need = a.model == 1 ? 4 : 3;
    for (int it = 0; it < a.lo_iters; ++it) {
        if (n_cur < need) { flags |= 2; break; }
        // Hartley normalisation over the masked pairs: centroid to the origin, mean distance sqrt(2)
        double c4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int t = tid; t < rows; t += SPV_LO_THREADS)
            if (a.cur[t]) { const float4 p = a.pts[t]; c4[0] += (double)p.x; c4[1] += (double)p.y; c4[2] += (double)p.z; c4[3] += (double)p.w; }
        spv_block_sum<4>(c4, s_part, s_sum);
        const double nn = (double)n_cur;
        const double cx1 = c4[0] / nn, cy1 = c4[1] / nn, cx2 = c4[2] / nn, cy2 = c4[3] / nn;
        double d2[2] = {0.0, 0.0};
        for (int t = tid; t < rows; t += SPV_LO_THREADS)
            if (a.cur[t]) {
                const float4 p = a.pts[t];
                const double ax = (double)p.x - cx1, ay = (double)p.y - cy1, bx = (double)p.z - cx2, by = (double)p.w - cy2;
                d2[0] += sqrt(ax * ax + ay * ay); d2[1] += sqrt(bx * bx + by * by);
            }
        spv_block_sum<2>(d2, s_part, s_sum);
        const double md1 = d2[0] / nn, md2 = d2[1] / nn;
        if (!(md1 > 0.0 && md2 > 0.0)) { flags |= 4; break; }      // all points of one image coincide
        const double s1 = 1.4142135623730951 / md1, s2 = 1.4142135623730951 / md2;
        if (a.model == 1) {
            // inhomogeneous DLT, h33 = 1: rows [x y 1 0 0 0 -xu -yu | u], [0 0 0 x y 1 -xv -yv | v]; normal equations M^T M h = M^T r
            double acc[SPV_NSUM];
#pragma unroll
            for (int k = 0; k < SPV_NSUM; ++k) acc[k] = 0.0;
            for (int t = tid; t < rows; t += SPV_LO_THREADS)
                if (a.cur[t]) {
                    const float4 p = a.pts[t];
                    const double x = ((double)p.x - cx1) * s1, y = ((double)p.y - cy1) * s1, u = ((double)p.z - cx2) * s2, w = ((double)p.w - cy2) * s2;
                    const double r1[8] = {x, y, 1.0, 0.0, 0.0, 0.0, -(x * u), -(y * u)};
                    const double r2[8] = {0.0, 0.0, 0.0, x, y, 1.0, -(x * w), -(y * w)};
                    int k = 0;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
#pragma unroll
                        for (int j = i; j < 8; ++j) { acc[k] += r1[i] * r1[j] + r2[i] * r2[j]; ++k; }
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[36 + i] += r1[i] * u + r2[i] * w;
                }
            spv_block_sum<SPV_NSUM>(acc, s_part, s_sum);
            if (tid == 0) {
                int k = 0;
                double dmax = 0.0;
                for (int i = 0; i < 8; ++i) {
                    for (int j = i; j < 8; ++j) { s_A[i * 9 + j] = s_sum[k]; s_A[j * 9 + i] = s_sum[k]; ++k; }
                    s_A[i * 9 + 8] = s_sum[36 + i];
                    dmax = fmax(dmax, fabs(s_A[i * 9 + i]));
                }
                const bool ok = spv_solve_lds(s_A, 8, 9, 1e-12 * dmax);
                double* Hn = s_m[0];
                for (int i = 0; i < 8; ++i) Hn[i] = s_A[i * 9 + 8];
                Hn[8] = 1.0;
                s_stop = ok ? 0 : 1;
            }
        } else {
            // affine: [x y 1] a = u, [x y 1] b = v: one 3 x 3 matrix S = sum p p^T, two right-hand sides
            double acc[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) acc[k] = 0.0;
            for (int t = tid; t < rows; t += SPV_LO_THREADS)
                if (a.cur[t]) {
                    const float4 p = a.pts[t];
                    const double x = ((double)p.x - cx1) * s1, y = ((double)p.y - cy1) * s1, u = ((double)p.z - cx2) * s2, w = ((double)p.w - cy2) * s2;
                    acc[0] += x * x; acc[1] += x * y; acc[2] += x; acc[3] += y * y; acc[4] += y; acc[5] += 1.0;
                    acc[6] += x * u; acc[7] += y * u; acc[8] += u; acc[9] += x * w; acc[10] += y * w; acc[11] += w;
                }
            spv_block_sum<12>(acc, s_part, s_sum);
            if (tid == 0) {
                // rows of [S | S^T-side right-hand sides], 3 x 5
                s_A[0] = s_sum[0]; s_A[1] = s_sum[1]; s_A[2] = s_sum[2]; s_A[3] = s_sum[6]; s_A[4] = s_sum[9];
                s_A[5] = s_sum[1]; s_A[6] = s_sum[3]; s_A[7] = s_sum[4]; s_A[8] = s_sum[7]; s_A[9] = s_sum[10];
                s_A[10] = s_sum[2]; s_A[11] = s_sum[4]; s_A[12] = s_sum[5]; s_A[13] = s_sum[8]; s_A[14] = s_sum[11];
                const double dmax = fmax(fmax(fabs(s_A[0]), fabs(s_A[6])), fabs(s_A[12]));
                const bool ok = spv_solve_lds(s_A, 3, 5, 1e-12 * dmax);
                double* Hn = s_m[0];
                Hn[0] = s_A[3]; Hn[1] = s_A[8]; Hn[2] = s_A[13];
                Hn[3] = s_A[4]; Hn[4] = s_A[9]; Hn[5] = s_A[14];
                Hn[6] = 0.0; Hn[7] = 0.0; Hn[8] = 1.0;
                s_stop = ok ? 0 : 1;
            }
        }
        if (tid == 0 && !s_stop) {
            // H = T2^-1 Hn T1, T = [s 0 -s cx; 0 s -s cy; 0 0 1], then H[2][2] = 1
            double* T1 = s_m[2];
            double* T2i = s_m[3];
            T1[0] = s1; T1[1] = 0.0; T1[2] = -s1 * cx1; T1[3] = 0.0; T1[4] = s1; T1[5] = -s1 * cy1; T1[6] = 0.0; T1[7] = 0.0; T1[8] = 1.0;
            T2i[0] = 1.0 / s2; T2i[1] = 0.0; T2i[2] = cx2; T2i[3] = 0.0; T2i[4] = 1.0 / s2; T2i[5] = cy2; T2i[6] = 0.0; T2i[7] = 0.0; T2i[8] = 1.0;
            spv_mul3_lds(s_m[0], T1, s_A);
            spv_mul3_lds(T2i, s_A, s_m[0]);
            const double h22 = s_m[0][8];
            bool ok = fabs(h22) > 0.0;
            for (int i = 0; i < 9; ++i) { s_m[0][i] = s_m[0][i] / h22; ok = ok && fabs(s_m[0][i]) <= 1.7976931348623157e308; }
            if (!ok) s_stop = 1;
        }
        __syncthreads();
        if (s_stop) { flags |= 4; break; }
        // the mask of this model: fp64 transfer error, w > 0
        double H[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) H[i] = s_m[0][i];
        double v[1] = {0.0};
        for (int t = tid; t < rows; t += SPV_LO_THREADS) {
            const float4 p = a.pts[t];
            const double x = p.x, y = p.y;
            const double w = (H[6] * x + H[7] * y) + H[8];
            const double px = ((H[0] * x + H[1] * y) + H[2]) / w - (double)p.z, py = ((H[3] * x + H[4] * y) + H[5]) / w - (double)p.w;
            const bool in = w > 0.0 && (px * px + py * py) <= th2;
            a.cur[t] = in;
            v[0] += in ? 1.0 : 0.0;
        }
        spv_block_sum<1>(v, s_part, s_sum);
        n_cur = (int)v[0];
        if (n_cur > n_best) {              // strict: on a tie the earliest model stays
            n_best = n_cur;
            for (int t = tid; t < rows; t += SPV_LO_THREADS) a.inlier[t] = a.cur[t];
            if (tid < 9) s_m[1][tid] = s_m[0][tid];
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid < 9) a.model_out[tid] = s_m[1][tid];
    if (tid == 0) { a.summary[0] = best; a.summary[1] = a.best[1]; a.summary[2] = n_best; a.summary[3] = flags; }
}

__global__ __launch_bounds__(SPV_LO_THREADS) void spv_lo_kernel(SpvLo a) { spv_lo_body(a); }

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// scratch: pts float4 [t_max] | hyp float4 [t_max] | best int32 [2] (+ pad to 16) | current mask uint8 [t_max]
extern "C" size_t affnet_verify_scratch_bytes(int t_max) {
    const size_t t = t_max > 0 ? (size_t)t_max : 0;
    return 2 * t * sizeof(float4) + 16 + aff_align(t, 16) + 64;
}

static int spv_check(affnet_ctx* ctx, const char* what, const void* d_lafs1, int n1, const void* d_lafs2, int n2, const void* d_tent, int t_max, float inl_th,
                     const void* d_counts, const void* d_scratch) {
    if (!ctx || !d_lafs1 || !d_lafs2 || !d_tent || !d_counts || !d_scratch || n1 < 0 || n2 < 0 || t_max < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: bad argument", what);
    if (((uintptr_t)d_scratch & 15) != 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: d_scratch must be 16-byte aligned", what);
    if (!(inl_th > 0.0f) || !(fabsf(inl_th) <= 3.402823466e38f)) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: inl_th must be finite and > 0", what);
    return AFFNET_OK;
}

// prep + score + select; d_best (int32[2]) may be the scratch slot
static int spv_score_launch(const SpvIn& in, float inl_th, int32_t* d_counts, int32_t* d_best, float4* pts, float4* hyp, hipStream_t st) {
    const int t_max = in.t_max;
    if (t_max > 0) {
        hipLaunchKernelGGL(spv_prep_kernel, dim3(aff_cdiv(t_max, 256)), dim3(256), 0, st, in, pts, hyp, d_counts);
        hipLaunchKernelGGL(spv_score_kernel, dim3(aff_cdiv(t_max, SPV_HT), aff_cdiv(t_max, SPV_MC)), dim3(SPV_HT), 0, st, (const float4*)pts, (const float4*)hyp,
                           in.count, t_max, inl_th * inl_th, d_counts);
    }
    hipLaunchKernelGGL(spv_select_kernel, dim3(1), dim3(256), 0, st, (const int32_t*)d_counts, in.count, t_max, d_best);
    return AFFNET_OK;
}

extern "C" int affnet_verify_score(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent, const int32_t* d_count,
                                   int t_max, float inl_th, int32_t* d_counts, int32_t* d_best, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    { int rc = spv_check(ctx, "verify_score", d_lafs1, n1, d_lafs2, n2, d_tent, t_max, inl_th, d_counts, d_scratch); if (rc) return rc; }
    if (!d_best) return aff_fail(ctx, AFFNET_ERR_INVALID, "verify_score: bad argument");
    const SpvIn in = {d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max};
    float4* pts = (float4*)d_scratch;
    spv_score_launch(in, inl_th, d_counts, d_best, pts, pts + t_max, (hipStream_t)stream);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

extern "C" int affnet_verify_matches(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent, const int32_t* d_count,
                                     int t_max, float inl_th, int model, int lo_iters, int32_t* d_counts, double* d_model, uint8_t* d_inlier, int32_t* d_summary,
                                     void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    { int rc = spv_check(ctx, "verify_matches", d_lafs1, n1, d_lafs2, n2, d_tent, t_max, inl_th, d_counts, d_scratch); if (rc) return rc; }
    if (!d_model || !d_inlier || !d_summary) return aff_fail(ctx, AFFNET_ERR_INVALID, "verify_matches: bad argument");
    if (model != AFFNET_VERIFY_AFFINE && model != AFFNET_VERIFY_HOMOGRAPHY)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "verify_matches: model %d (0 = affine, 1 = homography)", model);
    if (lo_iters < 0 || lo_iters > 8) return aff_fail(ctx, AFFNET_ERR_INVALID, "verify_matches: lo_iters %d outside 0..8", lo_iters);
    hipStream_t st = (hipStream_t)stream;
    const SpvIn in = {d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max};
    float4* pts = (float4*)d_scratch;
    float4* hyp = pts + t_max;
    int32_t* best = (int32_t*)(hyp + t_max);
    uint8_t* cur = (uint8_t*)best + 16;
    spv_score_launch(in, inl_th, d_counts, best, pts, hyp, st);
    SpvLo lo;
    lo.in = in; lo.pts = pts; lo.hyp = hyp; lo.best = best; lo.th = inl_th; lo.model = model; lo.lo_iters = lo_iters; lo.cur = cur;
    lo.model_out = d_model; lo.inlier = d_inlier; lo.summary = d_summary;
    hipLaunchKernelGGL(spv_lo_kernel, dim3(1), dim3(SPV_LO_THREADS), 0, st, lo);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// ---- many pairs in one call: the pair index on a grid dimension of every stage --------------------------------------------------------------
// A shortlist of P image pairs is P independent verifications: P x the workgroups of the scoring kernel and P concurrent local optimisations in
// the four launches of one pair.  Every kernel reads its row of the pair table, tests it (aff_pair_row, before any load through it), builds the
// pair's SpvIn from the segments and runs the single-pair body above: per pair the outputs are affnet_verify_matches' bit for bit.
// The tentative lists are (P, t_max, 2) as affnet_match_snn_many writes them with n1_max = t_max, which is this call's cap on n1; n2 has none.
// SpvMany and spv_many_in (the pair's SpvIn from its table row) are in spatial_dev.h: epipolar.hip builds its pairs with them too.
// grid (t_max / 256, P)
__global__ __launch_bounds__(256) void spv_many_prep_kernel(SpvMany m, int32_t* __restrict__ counts) {
    const int p = blockIdx.y;
    SpvIn in;
    if (!spv_many_in(m, p, in)) return;
    const size_t o = (size_t)p * m.t_max;
    spv_prep_body(in, m.pts + o, m.hyp + o, counts + o, blockIdx.x);
}

// grid (t_max / SPV_HT, t_max / SPV_MC, P)
__global__ __launch_bounds__(SPV_HT) void spv_many_score_kernel(SpvMany m, float th2, int32_t* __restrict__ counts) {
    const int p = blockIdx.z;
    SpvIn in;
    if (!spv_many_in(m, p, in)) return;
    const size_t o = (size_t)p * m.t_max;
    spv_score_body(m.pts + o, m.hyp + o, in.count, m.t_max, th2, counts + o, blockIdx.x, blockIdx.y);
}

// grid (P); an out-of-range pair has no rows
__global__ __launch_bounds__(256) void spv_many_select_kernel(SpvMany m, const int32_t* __restrict__ counts) {
    const int p = blockIdx.x;
    SpvIn in;
    if (!spv_many_in(m, p, in)) return;
    spv_select_body(counts + (size_t)p * m.t_max, in.count, m.t_max, m.best + 4 * (size_t)p);
}

// grid (P)
__global__ __launch_bounds__(SPV_LO_THREADS) void spv_many_lo_kernel(SpvMany m, float th, int model, int lo_iters, uint8_t* __restrict__ cur, int cur_pitch,
                                                                     double* __restrict__ model_out, uint8_t* __restrict__ inlier, int32_t* __restrict__ summary) {
    const int p = blockIdx.x, tid = threadIdx.x;
    SpvLo a;
    if (!spv_many_in(m, p, a.in)) {        // identity, nothing of the mask, flags 1 | 8
        if (tid < 9) model_out[9 * (size_t)p + tid] = (tid % 4 == 0) ? 1.0 : 0.0;
        if (tid == 0) { int32_t* s = summary + 4 * (size_t)p; s[0] = -1; s[1] = 0; s[2] = 0; s[3] = 1 | AFFNET_VERIFY_FLAG_PAIR_RANGE; }
        return;
    }
    const size_t o = (size_t)p * m.t_max;
    a.pts = m.pts + o; a.hyp = m.hyp + o; a.best = m.best + 4 * (size_t)p;
    a.th = th; a.model = model; a.lo_iters = lo_iters;
    a.cur = cur + (size_t)p * cur_pitch;
    a.model_out = model_out + 9 * (size_t)p; a.inlier = inlier + o; a.summary = summary + 4 * (size_t)p;
    spv_lo_body(a);
}

// scratch: pts float4 (P, t_max) | hyp float4 (P, t_max) | best int32 (P, 4) | current mask uint8 (P, align16(t_max))
extern "C" size_t affnet_verify_many_scratch_bytes(int n_pairs, int t_max) {
    const size_t P = n_pairs > 0 ? (size_t)n_pairs : 0, t = t_max > 0 ? (size_t)t_max : 0;
    return P * (2 * t * sizeof(float4) + 16 + aff_align(t, 16)) + 64;
}

extern "C" int affnet_verify_matches_many(affnet_ctx* ctx, const float* d_lafs1, int rows1, const float* d_lafs2, int rows2, const int32_t* d_pairs, int n_pairs,
                                          const int32_t* d_tent, const int32_t* d_count, int t_max, float inl_th, int model, int lo_iters, int32_t* d_counts,
                                          double* d_model, uint8_t* d_inlier, int32_t* d_summary, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    { int rc = spv_check(ctx, "verify_matches_many", d_lafs1, rows1, d_lafs2, rows2, d_tent, t_max, inl_th, d_counts, d_scratch); if (rc) return rc; }
    if (!d_pairs || !d_model || !d_inlier || !d_summary || n_pairs < 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "verify_matches_many: bad argument");
    if (n_pairs > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "verify_matches_many: %d pairs (at most 65535 per call)", n_pairs);
    if (model != AFFNET_VERIFY_AFFINE && model != AFFNET_VERIFY_HOMOGRAPHY)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "verify_matches_many: model %d (0 = affine, 1 = homography)", model);
    if (lo_iters < 0 || lo_iters > 8) return aff_fail(ctx, AFFNET_ERR_INVALID, "verify_matches_many: lo_iters %d outside 0..8", lo_iters);
    if (n_pairs == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)n_pairs;
    const unsigned gp = (unsigned)n_pairs;
    SpvMany m;
    m.lafs1 = d_lafs1; m.rows1 = rows1; m.lafs2 = d_lafs2; m.rows2 = rows2; m.pairs = d_pairs; m.tent = d_tent; m.count = d_count; m.t_max = t_max;
    m.pts = (float4*)d_scratch;
    m.hyp = m.pts + P * t_max;
    m.best = (int32_t*)(m.hyp + P * t_max);
    uint8_t* cur = (uint8_t*)(m.best + 4 * P);
    if (t_max > 0) {
        hipLaunchKernelGGL(spv_many_prep_kernel, dim3(aff_cdiv(t_max, 256), gp), dim3(256), 0, st, m, d_counts);
        hipLaunchKernelGGL(spv_many_score_kernel, dim3(aff_cdiv(t_max, SPV_HT), aff_cdiv(t_max, SPV_MC), gp), dim3(SPV_HT), 0, st, m, inl_th * inl_th, d_counts);
    }
    hipLaunchKernelGGL(spv_many_select_kernel, dim3(gp), dim3(256), 0, st, m, (const int32_t*)d_counts);
    hipLaunchKernelGGL(spv_many_lo_kernel, dim3(gp), dim3(SPV_LO_THREADS), 0, st, m, inl_th, model, lo_iters, cur, (int)aff_align((size_t)t_max, 16), d_model,
                       d_inlier, d_summary);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
