// Epipolar verification of tentative matches from their local affine frames, for gfx950 ("epipolar verification").
//
// An affine frame is three point correspondences (centre, two axis tips), so three tentative matches give the nine of a linear 8-point solve.
// Hypothesis (s, r) is seeded by tentative s, its two partners come from a counter-based integer hash of (s, r, seed): T x rounds hypotheses,
// the same bytes on every run, no random-number state.  The rules are stated in include/affnet_hip.h; the design is spatial.hip's.
//
//   epi_prep_kernel    per tentative: the two frames through `tent` (spv_gather: indices tested before any load) -> pts[t] = the centres
//                      (x1, y1, x2, y2), frm[t] = the twelve numbers; NaN for a match / member that is not usable.
//   epi_solve_kernel   one thread per hypothesis, fp64: members by the hash, Hartley normalisation of the nine points per image in registers,
//                      the 8 x 9 system in LDS as [element][thread] (runtime pivot indices address LDS, not a per-thread array, so the
//                      kernel has no scratch; a lane's doubles of one element are contiguous, so no bank conflict), complete pivoting,
//                      back-substitution, denormalisation -> hyp[h] nine fp32, counts[h] = 0.
//   epi_score_kernel   2-D grid (hypothesis tile EPI_HT) x (match chunk EPI_MC), F in registers, the chunk's centres in LDS read as a
//                      broadcast, one integer atomicAdd per thread and chunk.
//   epi_select_kernel  spv_select_rows over the T x rounds counts.
//   epi_lo_kernel      one workgroup, fp64: refits on the inliers of the best hypothesis - 9 x 9 normal matrix by the fixed-order sums of
//                      spv_block_sum, cyclic Jacobi by one thread on matrices held in LDS, rank 2 through a second 3 x 3 Jacobi.
//
// affnet_epipolar_verify_many (end of the file) runs the same five stages for P image pairs per launch: epi_many_*_kernel take the pair index
// from the grid, find the pair's segments in a device table (spv_many_in) and call the bodies of the kernels above.
// The hash, the scoring and selection bodies, the unit norm and the Jacobi are in epipolar_dev.h: epipolar_planar.hip runs them too.
#include "epipolar_dev.h"

#define EPI_NSUM 45         // upper triangle of the 9 x 9 normal matrix

// members m[1], m[2] of hypothesis (s, r); T >= 3
__device__ __forceinline__ void epi_members(uint32_t s, uint32_t r, uint32_t seed, uint32_t T, int (&m)[3]) {
    m[0] = (int)s;
#pragma unroll
    for (int k = 1; k <= 2; ++k) {
        const uint32_t x = epi_member_hash(s, r, (uint32_t)k, seed);
        uint32_t j = (uint32_t)(((uint64_t)x * T) >> 32);
        while (j == (uint32_t)m[0] || (k == 2 && j == (uint32_t)m[1])) j = (j + 1) % T;      // at most two steps: T >= 3
        m[k] = (int)j;
    }
}

// F = T2^T Fn T1, T = [s 0 -s cx; 0 s -s cy; 0 0 1], then unit Frobenius norm and the sign that makes the largest-magnitude entry (the first
// in row-major order on ties) positive.  false: the norm is zero or not finite.
__device__ __forceinline__ bool epi_denormalise(double (&F)[9], double s1, double cx1, double cy1, double s2, double cx2, double cy2) {
    const double tx1 = -s1 * cx1, ty1 = -s1 * cy1, tx2 = -s2 * cx2, ty2 = -s2 * cy2;
    double G[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = F[3 * r] * s1;
        G[3 * r + 1] = F[3 * r + 1] * s1;
        G[3 * r + 2] = (F[3 * r] * tx1 + F[3 * r + 1] * ty1) + F[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        F[c] = s2 * G[c];
        F[3 + c] = s2 * G[3 + c];
        F[6 + c] = (tx2 * G[c] + ty2 * G[3 + c]) + G[6 + c];
    }
    return epi_unit_sign(F);
}

// ---- prep -----------------------------------------------------------------------------------------------------------------------------
// frm: three float4 per row = (a b x c) (d y a2 b2) (x2 c2 d2 y2), i.e. the twelve numbers in frame order
// The *_body functions are the kernels of one image pair; the __global__ kernels, single-pair here and batched at the end of the file (pair index on
// a grid dimension), only choose the pointers and the workgroup indices they run on.
__device__ __forceinline__ void epi_prep_body(const SpvIn& in, float4* __restrict__ pts, float4* __restrict__ frm, int blk) {
    const int t = blk * 256 + threadIdx.x;
    if (t >= spv_rows(in.count, in.t_max)) return;
    const float qn = __builtin_nanf("");
    float4 p = make_float4(qn, qn, qn, qn), f0 = p, f1 = p, f2 = p;
    float A[6], B[6];
    if (spv_gather(in, t, A, B)) {
        const bool centres = spv_centres_finite(A, B);
        if (centres) p = make_float4(A[2], A[5], B[2], B[5]);
        if (centres && spv_shapes_finite(A, B)) {
            f0 = make_float4(A[0], A[1], A[2], A[3]); f1 = make_float4(A[4], A[5], B[0], B[1]); f2 = make_float4(B[2], B[3], B[4], B[5]);
        }
    }
    pts[t] = p; frm[3 * (size_t)t] = f0; frm[3 * (size_t)t + 1] = f1; frm[3 * (size_t)t + 2] = f2;
}

__global__ __launch_bounds__(256) void epi_prep_kernel(SpvIn in, float4* __restrict__ pts, float4* __restrict__ frm) {
    epi_prep_body(in, pts, frm, blockIdx.x);
}

// ---- solve ----------------------------------------------------------------------------------------------------------------------------
#define EPI_A(r, c) s_A[((r) * 9 + (c)) * EPI_ST + tid]

__device__ __forceinline__ void epi_solve_body(const float4* __restrict__ frm, const int32_t* __restrict__ count, int t_max, int rounds, uint32_t seed,
                                               float* __restrict__ hyp, int32_t* __restrict__ counts, int blk) {
    __shared__ double s_A[72 * EPI_ST];
    __shared__ double s_f[9 * EPI_ST];
    __shared__ int s_perm[9 * EPI_ST];
    const int tid = threadIdx.x;
    const int rows = spv_rows(count, t_max);
    const long long h64 = (long long)blk * EPI_ST + tid;
    if (h64 >= (long long)rows * rounds) return;
    const int h = (int)h64;
    double F[9];
    bool ok = rows >= 3;
    if (ok) {
        int m[3];
        epi_members((uint32_t)(h / rounds), (uint32_t)(h % rounds), seed, (uint32_t)rows, m);
        // the nine points per image: member k's centre, tip 0 = centre + first column, tip 1 = centre + second column
        double X[9], Y[9], U[9], V[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 f0 = frm[3 * (size_t)m[k]], f1 = frm[3 * (size_t)m[k] + 1], f2 = frm[3 * (size_t)m[k] + 2];
            ok = ok && spv_finite(f0.x);                          // a member that is not usable has NaN in all twelve
            const double a = f0.x, b = f0.y, x = f0.z, c = f0.w, d = f1.x, y = f1.y;
            const double a2 = f1.z, b2 = f1.w, x2 = f2.x, c2 = f2.y, d2 = f2.z, y2 = f2.w;
            X[3 * k] = x; Y[3 * k] = y; X[3 * k + 1] = x + a; Y[3 * k + 1] = y + c; X[3 * k + 2] = x + b; Y[3 * k + 2] = y + d;
            U[3 * k] = x2; V[3 * k] = y2; U[3 * k + 1] = x2 + a2; V[3 * k + 1] = y2 + c2; U[3 * k + 2] = x2 + b2; V[3 * k + 2] = y2 + d2;
        }
        double cx1 = 0.0, cy1 = 0.0, cx2 = 0.0, cy2 = 0.0;
#pragma unroll
        for (int p = 0; p < 9; ++p) { cx1 += X[p]; cy1 += Y[p]; cx2 += U[p]; cy2 += V[p]; }
        cx1 = cx1 / 9.0; cy1 = cy1 / 9.0; cx2 = cx2 / 9.0; cy2 = cy2 / 9.0;
        double md1 = 0.0, md2 = 0.0;
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            const double ax = X[p] - cx1, ay = Y[p] - cy1, bx = U[p] - cx2, by = V[p] - cy2;
            md1 += sqrt(ax * ax + ay * ay); md2 += sqrt(bx * bx + by * by);
        }
        md1 = md1 / 9.0; md2 = md2 / 9.0;
        const double s1 = 1.4142135623730951 / md1, s2 = 1.4142135623730951 / md2;
        ok = ok && s1 > 0.0 && s2 > 0.0 && epi_finite(s1) && epi_finite(s2);
        if (ok) {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const double x = (X[p] - cx1) * s1, y = (Y[p] - cy1) * s1, u = (U[p] - cx2) * s2, v = (V[p] - cy2) * s2;
                EPI_A(p, 0) = u * x; EPI_A(p, 1) = u * y; EPI_A(p, 2) = u; EPI_A(p, 3) = v * x; EPI_A(p, 4) = v * y; EPI_A(p, 5) = v;
                EPI_A(p, 6) = x; EPI_A(p, 7) = y; EPI_A(p, 8) = 1.0;
            }
            for (int c = 0; c < 9; ++c) s_perm[c * EPI_ST + tid] = c;
            // elimination with complete pivoting; every index below addresses this thread's column of the LDS arrays
            for (int k = 0; k < 8 && ok; ++k) {
                int pr = k, pc = k;
                double pv = -1.0;
                for (int r = k; r < 8; ++r)
                    for (int c = k; c < 9; ++c) {
                        const double a = fabs(EPI_A(r, c));
                        if (a > pv) { pv = a; pr = r; pc = c; }           // strict: ties stay with the smallest row, then the smallest column
                    }
                if (!(pv >= 1e-12)) { ok = false; break; }
                if (pr != k)
                    for (int c = 0; c < 9; ++c) { const double t = EPI_A(k, c); EPI_A(k, c) = EPI_A(pr, c); EPI_A(pr, c) = t; }
                if (pc != k) {
                    for (int r = 0; r < 8; ++r) { const double t = EPI_A(r, k); EPI_A(r, k) = EPI_A(r, pc); EPI_A(r, pc) = t; }
                    const int t = s_perm[k * EPI_ST + tid]; s_perm[k * EPI_ST + tid] = s_perm[pc * EPI_ST + tid]; s_perm[pc * EPI_ST + tid] = t;
                }
                const double piv = EPI_A(k, k);
                for (int r = k + 1; r < 8; ++r) {
                    const double f = EPI_A(r, k) / piv;
                    for (int c = k + 1; c < 9; ++c) EPI_A(r, c) = EPI_A(r, c) - f * EPI_A(k, c);
                }
            }
        }
        if (ok) {
            // back-substitution with the free unknown (permuted column 8) = 1; y[i] replaces A[i][8]
            for (int i = 7; i >= 0; --i) {
                double s = EPI_A(i, 8);
                for (int j = i + 1; j < 8; ++j) s += EPI_A(i, j) * EPI_A(j, 8);
                EPI_A(i, 8) = -s / EPI_A(i, i);
            }
            for (int j = 0; j < 8; ++j) s_f[s_perm[j * EPI_ST + tid] * EPI_ST + tid] = EPI_A(j, 8);
            s_f[s_perm[8 * EPI_ST + tid] * EPI_ST + tid] = 1.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) F[i] = s_f[i * EPI_ST + tid];
            ok = epi_denormalise(F, s1, cx1, cy1, s2, cx2, cy2);
        }
    }
    float* out = hyp + 9 * (size_t)h;
    const float qn = __builtin_nanf("");
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = ok ? (float)F[i] : qn;
    counts[h] = 0;
}

__global__ __launch_bounds__(EPI_ST) void epi_solve_kernel(const float4* __restrict__ frm, const int32_t* __restrict__ count, int t_max, int rounds, uint32_t seed,
                                                           float* __restrict__ hyp, int32_t* __restrict__ counts) {
    epi_solve_body(frm, count, t_max, rounds, seed, hyp, counts, blockIdx.x);
}

// ---- score + select -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EPI_HT) void epi_score_kernel(const float4* __restrict__ pts, const float* __restrict__ hyp, const int32_t* __restrict__ count,
                                                           int t_max, int rounds, float th2, int32_t* __restrict__ counts) {
    epi_score_body(pts, hyp, count, t_max, rounds, th2, counts, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void epi_select_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ count, int t_max, int rounds,
                                                         int32_t* __restrict__ best) {
    epi_select_body(counts, count, t_max, rounds, best);
}

// ---- local optimisation ---------------------------------------------------------------------------------------------------------------
struct EpiLo {
    const int32_t* count; int t_max;
    const float4* pts; const float* hyp;
    const int32_t* best;       // {index, count} of epi_select_kernel
    float th; int lo_iters;
    uint8_t* cur;              // scratch: the current mask
    double* model_out; uint8_t* inlier; int32_t* summary;
};

__device__ __forceinline__ void epi_lo_body(const EpiLo& a) {
    __shared__ double s_part[4 * EPI_NSUM], s_sum[EPI_NSUM];
    __shared__ double s_N[81], s_V[81], s_M[9], s_W[9];
    __shared__ double s_m[2][9];           // 0: candidate model, 1: kept model
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    const int rows = spv_rows(a.count, a.t_max);
    const int best = a.best[0];
    if (best < 0) {                        // no valid hypothesis (or no rows): zero model, empty mask, flag 1
        for (int t = tid; t < rows; t += EPI_LO_THREADS) a.inlier[t] = 0;
        if (tid < 9) a.model_out[tid] = 0.0;
        if (tid == 0) { a.summary[0] = -1; a.summary[1] = 0; a.summary[2] = 0; a.summary[3] = 1; }
        return;
    }
    float Ff[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Ff[i] = a.hyp[9 * (size_t)best + i];
    if (tid < 9) s_m[1][tid] = (double)a.hyp[9 * (size_t)best + tid];      // model 0: the hypothesis itself
    if (tid == 0) s_stop = 0;
    const float th2f = a.th * a.th;
    const double th2 = (double)a.th * (double)a.th;
    int n_cur, n_best, flags = 0;
    {
        double v[1] = {0.0};
        for (int t = tid; t < rows; t += EPI_LO_THREADS) {
            const bool in = epi_inlier(Ff, a.pts[t], th2f);
            a.cur[t] = in; a.inlier[t] = in;           // thread tid owns rows tid, tid + 256, ... of both masks throughout
            v[0] += in ? 1.0 : 0.0;
        }
        spv_block_sum<1>(v, s_part, s_sum);
        n_cur = n_best = (int)v[0];
    }
    for (int it = 0; it < a.lo_iters; ++it) {
        if (n_cur < 8) { flags |= 2; break; }
        // Hartley normalisation over the masked centres
        double c4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int t = tid; t < rows; t += EPI_LO_THREADS)
            if (a.cur[t]) { const float4 p = a.pts[t]; c4[0] += (double)p.x; c4[1] += (double)p.y; c4[2] += (double)p.z; c4[3] += (double)p.w; }
        spv_block_sum<4>(c4, s_part, s_sum);
        const double nn = (double)n_cur;
        const double cx1 = c4[0] / nn, cy1 = c4[1] / nn, cx2 = c4[2] / nn, cy2 = c4[3] / nn;
        double d2[2] = {0.0, 0.0};
        for (int t = tid; t < rows; t += EPI_LO_THREADS)
            if (a.cur[t]) {
                const float4 p = a.pts[t];
                const double ax = (double)p.x - cx1, ay = (double)p.y - cy1, bx = (double)p.z - cx2, by = (double)p.w - cy2;
                d2[0] += sqrt(ax * ax + ay * ay); d2[1] += sqrt(bx * bx + by * by);
            }
        spv_block_sum<2>(d2, s_part, s_sum);
        const double s1 = 1.4142135623730951 / (d2[0] / nn), s2 = 1.4142135623730951 / (d2[1] / nn);
        if (!(s1 > 0.0 && s2 > 0.0 && epi_finite(s1) && epi_finite(s2))) { flags |= 4; break; }      // all points of one image coincide
        // N = A^T A, upper triangle
        double acc[EPI_NSUM];
#pragma unroll
        for (int k = 0; k < EPI_NSUM; ++k) acc[k] = 0.0;
        for (int t = tid; t < rows; t += EPI_LO_THREADS)
            if (a.cur[t]) {
                const float4 p = a.pts[t];
                const double x = ((double)p.x - cx1) * s1, y = ((double)p.y - cy1) * s1, u = ((double)p.z - cx2) * s2, v = ((double)p.w - cy2) * s2;
                const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
                int k = 0;
#pragma unroll
                for (int i = 0; i < 9; ++i) {
#pragma unroll
                    for (int j = i; j < 9; ++j) { acc[k] += r[i] * r[j]; ++k; }
                }
            }
        spv_block_sum<EPI_NSUM>(acc, s_part, s_sum);
        if (tid == 0) {
            int k = 0;
            for (int i = 0; i < 9; ++i)
                for (int j = i; j < 9; ++j) { s_N[i * 9 + j] = s_sum[k]; s_N[j * 9 + i] = s_sum[k]; ++k; }
            epi_jacobi_lds<9>(s_N, s_V);
            int e;
            bool ok = epi_smallest(s_N, 9, true, e);
            if (ok) {
                // rank 2: Fn <- Fn - (Fn v) v^T, v the smallest eigenvector of Fn^T Fn
                double* Fn = s_m[0];
                for (int i = 0; i < 9; ++i) Fn[i] = s_V[i * 9 + e];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) s_M[3 * i + j] = (Fn[i] * Fn[j] + Fn[3 + i] * Fn[3 + j]) + Fn[6 + i] * Fn[6 + j];
                epi_jacobi_lds<3>(s_M, s_W);
                int e3;
                ok = epi_smallest(s_M, 3, false, e3);
                const double v0 = s_W[e3], v1 = s_W[3 + e3], v2 = s_W[6 + e3];
                for (int r = 0; r < 3; ++r) {
                    const double w = (Fn[3 * r] * v0 + Fn[3 * r + 1] * v1) + Fn[3 * r + 2] * v2;
                    Fn[3 * r] = Fn[3 * r] - w * v0; Fn[3 * r + 1] = Fn[3 * r + 1] - w * v1; Fn[3 * r + 2] = Fn[3 * r + 2] - w * v2;
                }
            }
            s_stop = ok ? 0 : 1;
        }
        __syncthreads();
        if (s_stop) { flags |= 4; break; }
        double F[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = s_m[0][i];
        const bool fin = epi_denormalise(F, s1, cx1, cy1, s2, cx2, cy2);      // every thread, the same numbers
        if (!fin) { flags |= 4; break; }
        double v[1] = {0.0};
        for (int t = tid; t < rows; t += EPI_LO_THREADS) {
            const bool in = epi_inlier64(F, a.pts[t], th2);
            a.cur[t] = in;
            v[0] += in ? 1.0 : 0.0;
        }
        spv_block_sum<1>(v, s_part, s_sum);
        n_cur = (int)v[0];
        if (n_cur > n_best) {              // strict: on a tie the earliest model stays
            n_best = n_cur;
            for (int t = tid; t < rows; t += EPI_LO_THREADS) a.inlier[t] = a.cur[t];
            if (tid < 9) s_m[1][tid] = F[tid];
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid < 9) a.model_out[tid] = s_m[1][tid];
    if (tid == 0) { a.summary[0] = best; a.summary[1] = a.best[1]; a.summary[2] = n_best; a.summary[3] = flags; }
}

__global__ __launch_bounds__(EPI_LO_THREADS) void epi_lo_kernel(EpiLo a) { epi_lo_body(a); }

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// scratch: pts float4 [t_max] | frm float4 [3 t_max] | hyp float [9 t_max rounds] (+ pad to 16) | best int32 [2] (+ pad to 16) | current mask uint8 [t_max]
static size_t epi_hyp_bytes(size_t t, size_t rounds) { return aff_align(9 * t * rounds * sizeof(float), 16); }

extern "C" size_t affnet_epipolar_scratch_bytes(int t_max, int rounds) {
    const size_t t = t_max > 0 ? (size_t)t_max : 0, r = rounds > 0 ? (size_t)rounds : 0;
    return 4 * t * sizeof(float4) + epi_hyp_bytes(t, r) + 16 + aff_align(t, 16) + 64;
}

static int epi_check(affnet_ctx* ctx, const char* what, const void* d_lafs1, int n1, const void* d_lafs2, int n2, const void* d_tent, int t_max, float inl_th,
                     int rounds, const void* d_counts, const void* d_scratch) {
    if (!ctx || !d_lafs1 || !d_lafs2 || !d_tent || !d_counts || !d_scratch || n1 < 0 || n2 < 0 || t_max < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: bad argument", what);
    if (((uintptr_t)d_scratch & 15) != 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: d_scratch must be 16-byte aligned", what);
    if (!(inl_th > 0.0f) || !(fabsf(inl_th) <= 3.402823466e38f)) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: inl_th must be finite and > 0", what);
    if (rounds < 1 || rounds > AFFNET_EPI_MAX_ROUNDS) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: rounds %d outside 1..%d", what, rounds, AFFNET_EPI_MAX_ROUNDS);
    if ((long long)t_max * rounds > 0x7fffffffLL) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: t_max * rounds = %lld hypotheses (at most 2^31 - 1)", what, (long long)t_max * rounds);
    return AFFNET_OK;
}

struct EpiBuf { float4* pts; float4* frm; float* hyp; int32_t* best; uint8_t* cur; };

static EpiBuf epi_carve(void* d_scratch, int t_max, int rounds) {
    EpiBuf b;
    b.pts = (float4*)d_scratch;
    b.frm = b.pts + t_max;
    b.hyp = (float*)(b.frm + 3 * (size_t)t_max);
    b.best = (int32_t*)((char*)b.hyp + epi_hyp_bytes((size_t)t_max, (size_t)rounds));
    b.cur = (uint8_t*)b.best + 16;
    return b;
}

// prep + solve + score + select
static void epi_score_launch(const SpvIn& in, float inl_th, int rounds, uint32_t seed, const EpiBuf& b, float* hyp, int32_t* d_counts, int32_t* d_best, hipStream_t st) {
    const int t_max = in.t_max;
    if (t_max > 0) {
        const int nh = t_max * rounds;
        hipLaunchKernelGGL(epi_prep_kernel, dim3(aff_cdiv(t_max, 256)), dim3(256), 0, st, in, b.pts, b.frm);
        hipLaunchKernelGGL(epi_solve_kernel, dim3(aff_cdiv(nh, EPI_ST)), dim3(EPI_ST), 0, st, (const float4*)b.frm, in.count, t_max, rounds, seed, hyp, d_counts);
        hipLaunchKernelGGL(epi_score_kernel, dim3(aff_cdiv(nh, EPI_HT), aff_cdiv(t_max, EPI_MC)), dim3(EPI_HT), 0, st, (const float4*)b.pts, (const float*)hyp,
                           in.count, t_max, rounds, inl_th * inl_th, d_counts);
    }
    hipLaunchKernelGGL(epi_select_kernel, dim3(1), dim3(256), 0, st, (const int32_t*)d_counts, in.count, t_max, rounds, d_best);
}

extern "C" int affnet_epipolar_score(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent, const int32_t* d_count,
                                     int t_max, float inl_th, int rounds, uint32_t seed, float* d_hyp, int32_t* d_counts, int32_t* d_best, void* d_scratch,
                                     void* stream) {
    AFF_DEVICE(ctx);
    { int rc = epi_check(ctx, "epipolar_score", d_lafs1, n1, d_lafs2, n2, d_tent, t_max, inl_th, rounds, d_counts, d_scratch); if (rc) return rc; }
    if (!d_best) return aff_fail(ctx, AFFNET_ERR_INVALID, "epipolar_score: bad argument");
    const SpvIn in = {d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max};
    const EpiBuf b = epi_carve(d_scratch, t_max, rounds);
    epi_score_launch(in, inl_th, rounds, seed, b, d_hyp ? d_hyp : b.hyp, d_counts, d_best, (hipStream_t)stream);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

extern "C" int affnet_epipolar_verify(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent, const int32_t* d_count,
                                      int t_max, float inl_th, int rounds, uint32_t seed, int lo_iters, int32_t* d_counts, double* d_model, uint8_t* d_inlier,
                                      int32_t* d_summary, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    { int rc = epi_check(ctx, "epipolar_verify", d_lafs1, n1, d_lafs2, n2, d_tent, t_max, inl_th, rounds, d_counts, d_scratch); if (rc) return rc; }
    if (!d_model || !d_inlier || !d_summary) return aff_fail(ctx, AFFNET_ERR_INVALID, "epipolar_verify: bad argument");
    if (lo_iters < 0 || lo_iters > 8) return aff_fail(ctx, AFFNET_ERR_INVALID, "epipolar_verify: lo_iters %d outside 0..8", lo_iters);
    hipStream_t st = (hipStream_t)stream;
    const SpvIn in = {d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max};
    const EpiBuf b = epi_carve(d_scratch, t_max, rounds);
    epi_score_launch(in, inl_th, rounds, seed, b, b.hyp, d_counts, b.best, st);
    EpiLo lo;
    lo.count = d_count; lo.t_max = t_max; lo.pts = b.pts; lo.hyp = b.hyp; lo.best = b.best; lo.th = inl_th; lo.lo_iters = lo_iters; lo.cur = b.cur;
    lo.model_out = d_model; lo.inlier = d_inlier; lo.summary = d_summary;
    hipLaunchKernelGGL(epi_lo_kernel, dim3(1), dim3(EPI_LO_THREADS), 0, st, lo);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// ---- many pairs in one call: the pair index on a grid dimension of every stage --------------------------------------------------------------
// One pair is latency: five dependent launches, the last of them one workgroup whose Jacobi sweeps run on one thread.  P pairs are P x the
// workgroups in the same five launches and P concurrent local optimisations.  Every kernel reads its row of the pair table, tests it
// (spv_many_in -> aff_pair_row, before any load through it), builds the pair's SpvIn from the segments and runs the single-pair body above: per
// pair the outputs are affnet_epipolar_verify's bit for bit.  SpvMany::hyp holds the frames here, (P, 3 t_max) float4.
struct EpiMany {
    SpvMany m;
    int rounds;
    float* hyp;                // scratch: (P, 9 t_max rounds)
    int32_t* counts;           // (P, t_max rounds)
};

__device__ __forceinline__ size_t epi_many_nh(const EpiMany& e) { return (size_t)e.m.t_max * e.rounds; }

// grid (t_max / 256, P)
__global__ __launch_bounds__(256) void epi_many_prep_kernel(EpiMany e) {
    const int p = blockIdx.y;
    SpvIn in;
    if (!spv_many_in(e.m, p, in)) return;
    const size_t o = (size_t)p * e.m.t_max;
    epi_prep_body(in, e.m.pts + o, e.m.hyp + 3 * o, blockIdx.x);
}

// grid (t_max rounds / EPI_ST, P)
__global__ __launch_bounds__(EPI_ST) void epi_many_solve_kernel(EpiMany e, uint32_t seed) {
    const int p = blockIdx.y;
    SpvIn in;
    if (!spv_many_in(e.m, p, in)) return;
    const size_t oh = (size_t)p * epi_many_nh(e);
    epi_solve_body(e.m.hyp + 3 * (size_t)p * e.m.t_max, in.count, e.m.t_max, e.rounds, seed, e.hyp + 9 * oh, e.counts + oh, blockIdx.x);
}

// grid (t_max rounds / EPI_HT, t_max / EPI_MC, P)
__global__ __launch_bounds__(EPI_HT) void epi_many_score_kernel(EpiMany e, float th2) {
    const int p = blockIdx.z;
    SpvIn in;
    if (!spv_many_in(e.m, p, in)) return;
    const size_t oh = (size_t)p * epi_many_nh(e);
    epi_score_body(e.m.pts + (size_t)p * e.m.t_max, e.hyp + 9 * oh, in.count, e.m.t_max, e.rounds, th2, e.counts + oh, blockIdx.x, blockIdx.y);
}

// grid (P); an out-of-range pair has no rows
__global__ __launch_bounds__(256) void epi_many_select_kernel(EpiMany e) {
    const int p = blockIdx.x;
    SpvIn in;
    if (!spv_many_in(e.m, p, in)) return;
    epi_select_body(e.counts + (size_t)p * epi_many_nh(e), in.count, e.m.t_max, e.rounds, e.m.best + 4 * (size_t)p);
}

// grid (P)
__global__ __launch_bounds__(EPI_LO_THREADS) void epi_many_lo_kernel(EpiMany e, float th, int lo_iters, uint8_t* __restrict__ cur, int cur_pitch,
                                                                     double* __restrict__ model_out, uint8_t* __restrict__ inlier, int32_t* __restrict__ summary) {
    const int p = blockIdx.x, tid = threadIdx.x;
    SpvIn in;
    if (!spv_many_in(e.m, p, in)) {        // the zero model of flag 1, nothing of the mask, flags 1 | 8
        if (tid < 9) model_out[9 * (size_t)p + tid] = 0.0;
        if (tid == 0) { int32_t* s = summary + 4 * (size_t)p; s[0] = -1; s[1] = 0; s[2] = 0; s[3] = 1 | AFFNET_VERIFY_FLAG_PAIR_RANGE; }
        return;
    }
    const size_t o = (size_t)p * e.m.t_max;
    EpiLo a;
    a.count = in.count; a.t_max = e.m.t_max; a.pts = e.m.pts + o; a.hyp = e.hyp + 9 * (size_t)p * epi_many_nh(e); a.best = e.m.best + 4 * (size_t)p;
    a.th = th; a.lo_iters = lo_iters;
    a.cur = cur + (size_t)p * cur_pitch;
    a.model_out = model_out + 9 * (size_t)p; a.inlier = inlier + o; a.summary = summary + 4 * (size_t)p;
    epi_lo_body(a);
}

// scratch: pts float4 (P, t_max) | frm float4 (P, 3 t_max) | hyp float (P, 9 t_max rounds) in P x epi_hyp_bytes | best int32 (P, 4) |
// current mask uint8 (P, align16(t_max))
extern "C" size_t affnet_epipolar_many_scratch_bytes(int n_pairs, int t_max, int rounds) {
    const size_t P = n_pairs > 0 ? (size_t)n_pairs : 0, t = t_max > 0 ? (size_t)t_max : 0, r = rounds > 0 ? (size_t)rounds : 0;
    return P * (4 * t * sizeof(float4) + epi_hyp_bytes(t, r) + 16 + aff_align(t, 16)) + 64;
}

extern "C" int affnet_epipolar_verify_many(affnet_ctx* ctx, const float* d_lafs1, int rows1, const float* d_lafs2, int rows2, const int32_t* d_pairs, int n_pairs,
                                           const int32_t* d_tent, const int32_t* d_count, int t_max, float inl_th, int rounds, uint32_t seed, int lo_iters,
                                           int32_t* d_counts, double* d_model, uint8_t* d_inlier, int32_t* d_summary, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    { int rc = epi_check(ctx, "epipolar_verify_many", d_lafs1, rows1, d_lafs2, rows2, d_tent, t_max, inl_th, rounds, d_counts, d_scratch); if (rc) return rc; }
    if (!d_pairs || !d_model || !d_inlier || !d_summary || n_pairs < 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "epipolar_verify_many: bad argument");
    if (n_pairs > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "epipolar_verify_many: %d pairs (at most 65535 per call)", n_pairs);
    if (lo_iters < 0 || lo_iters > 8) return aff_fail(ctx, AFFNET_ERR_INVALID, "epipolar_verify_many: lo_iters %d outside 0..8", lo_iters);
    if (n_pairs == 0) return AFFNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)n_pairs;
    const unsigned gp = (unsigned)n_pairs;
    EpiMany e;
    e.m.lafs1 = d_lafs1; e.m.rows1 = rows1; e.m.lafs2 = d_lafs2; e.m.rows2 = rows2; e.m.pairs = d_pairs; e.m.tent = d_tent; e.m.count = d_count; e.m.t_max = t_max;
    e.m.pts = (float4*)d_scratch;
    e.m.hyp = e.m.pts + P * t_max;
    e.hyp = (float*)(e.m.hyp + 3 * P * t_max);
    e.m.best = (int32_t*)((char*)e.hyp + P * epi_hyp_bytes((size_t)t_max, (size_t)rounds));
    uint8_t* cur = (uint8_t*)(e.m.best + 4 * P);
    e.rounds = rounds; e.counts = d_counts;
    if (t_max > 0) {
        const int nh = t_max * rounds;
        hipLaunchKernelGGL(epi_many_prep_kernel, dim3(aff_cdiv(t_max, 256), gp), dim3(256), 0, st, e);
        hipLaunchKernelGGL(epi_many_solve_kernel, dim3(aff_cdiv(nh, EPI_ST), gp), dim3(EPI_ST), 0, st, e, seed);
        hipLaunchKernelGGL(epi_many_score_kernel, dim3(aff_cdiv(nh, EPI_HT), aff_cdiv(t_max, EPI_MC), gp), dim3(EPI_HT), 0, st, e, inl_th * inl_th);
    }
    hipLaunchKernelGGL(epi_many_select_kernel, dim3(gp), dim3(256), 0, st, e);
    hipLaunchKernelGGL(epi_many_lo_kernel, dim3(gp), dim3(EPI_LO_THREADS), 0, st, e, inl_th, lo_iters, cur, (int)aff_align((size_t)t_max, 16), d_model, d_inlier,
                       d_summary);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
