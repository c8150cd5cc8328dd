// Device functions shared by the two epipolar verification files: epipolar.hip (the 8-point model from affine frames) and epipolar_planar.hip
// (plane-and-parallax: F = [e]x H from the dominant plane's homography).  The hash, the scoring rule, the selection, the unit norm with its
// sign rule and the cyclic Jacobi are written here once; both files are built with -ffp-contract=off (no fused multiply-add).
#pragma once
#include <math.h>

#include "common.h"
#include "spatial_dev.h"

#define EPI_HT 128          // hypotheses per workgroup of the scoring kernel = its workgroup size (AFFNET_EPI_TILE)
#define EPI_MC 128          // matches per LDS chunk (AFFNET_EPI_CHUNK)
#define EPI_ST 64           // hypotheses per workgroup of the solve kernel (AFFNET_EPI_SOLVE_TILE)
#define EPI_LO_THREADS 256
#define EPI_SWEEPS 12
#define EPI_DBL_MAX 1.7976931348623157e308

static_assert(EPI_HT == AFFNET_EPI_TILE && EPI_MC == AFFNET_EPI_CHUNK && EPI_ST == AFFNET_EPI_SOLVE_TILE, "include/affnet_hip.h states the tile sizes");

__device__ __forceinline__ bool epi_finite(double x) { return fabs(x) <= EPI_DBL_MAX; }

__device__ __forceinline__ uint32_t epi_lowbias32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// the hash of (s, r, k, seed) that picks member k of hypothesis (s, r)
__device__ __forceinline__ uint32_t epi_member_hash(uint32_t s, uint32_t r, uint32_t k, uint32_t seed) {
    return epi_lowbias32((s * 0x9E3779B1u) ^ (r * 0x85EBCA77u) ^ (k * 0xC2B2AE3Du) ^ seed);
}

// The scoring rule, fp32 (no fused multiply-add): Sampson error of the centres <= th^2
__device__ __forceinline__ bool epi_inlier(const float (&F)[9], const float4 p, float th2) {
    const float x = p.x, y = p.y, u = p.z, v = p.w;
    const float l0 = (F[0] * x + F[1] * y) + F[2], l1 = (F[3] * x + F[4] * y) + F[5], l2 = (F[6] * x + F[7] * y) + F[8];
    const float m0 = (F[0] * u + F[3] * v) + F[6], m1 = (F[1] * u + F[4] * v) + F[7];
    const float r = (u * l0 + v * l1) + l2;
    const float e = (r * r) / (((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1);
    return e <= th2;
}

// the same expression tree in fp64
__device__ __forceinline__ bool epi_inlier64(const double (&F)[9], const float4 p, double th2) {
    const double x = p.x, y = p.y, u = p.z, v = p.w;
    const double l0 = (F[0] * x + F[1] * y) + F[2], l1 = (F[3] * x + F[4] * y) + F[5], l2 = (F[6] * x + F[7] * y) + F[8];
    const double m0 = (F[0] * u + F[3] * v) + F[6], m1 = (F[1] * u + F[4] * v) + F[7];
    const double r = (u * l0 + v * l1) + l2;
    const double e = (r * r) / (((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1);
    return e <= th2;
}

// Unit Frobenius norm and the sign that makes the largest-magnitude entry (the first in row-major order on ties) positive.
// false: the norm is zero or not finite.
__device__ __forceinline__ bool epi_unit_sign(double (&F)[9]) {
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) n2 += F[i] * F[i];
    const double n = sqrt(n2);
    if (!(n > 0.0) || !epi_finite(n)) return false;
    double big = 0.0, sign = 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        F[i] = F[i] / n;
        if (fabs(F[i]) > big) { big = fabs(F[i]); sign = F[i] < 0.0 ? -1.0 : 1.0; }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = sign * F[i];
    return true;
}

// ---- score + select -------------------------------------------------------------------------------------------------------------------
// nh hypotheses against `rows` matches: workgroup (blk_h, blk_t) adds its chunk's inliers to counts[h]
__device__ __forceinline__ void epi_score_rows(const float4* __restrict__ pts, const float* __restrict__ hyp, int rows, long long nh, float th2,
                                               int32_t* __restrict__ counts, int blk_h, int blk_t) {
    __shared__ float4 s_pt[EPI_MC];
    const long long h0 = (long long)blk_h * EPI_HT;
    const int t0 = blk_t * EPI_MC;
    if (h0 >= nh || t0 >= rows) return;                       // uniform over the workgroup
    const int nt = min(EPI_MC, rows - t0);
    for (int k = threadIdx.x; k < nt; k += EPI_HT) s_pt[k] = pts[t0 + k];
    __syncthreads();
    const long long h = h0 + threadIdx.x;
    if (h >= nh) return;
    float F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = hyp[9 * (size_t)h + i];
    int c = 0;
    for (int k = 0; k < nt; ++k) c += epi_inlier(F, s_pt[k], th2) ? 1 : 0;
    if (c) atomicAdd(&counts[h], c);
}

// the 8-point call: rows x rounds hypotheses against the rows
__device__ __forceinline__ void epi_score_body(const float4* __restrict__ pts, const float* __restrict__ hyp, const int32_t* __restrict__ count, int t_max,
                                               int rounds, float th2, int32_t* __restrict__ counts, int blk_h, int blk_t) {
    const int rows = spv_rows(count, t_max);
    epi_score_rows(pts, hyp, rows, (long long)rows * rounds, th2, counts, blk_h, blk_t);
}

__device__ __forceinline__ void epi_select_body(const int32_t* __restrict__ counts, const int32_t* __restrict__ count, int t_max, int rounds,
                                                int32_t* __restrict__ best) {
    spv_select_rows(counts, spv_rows(count, t_max) * rounds, best);
}

// ---- eigenvectors ---------------------------------------------------------------------------------------------------------------------
// Cyclic Jacobi on the symmetric N x N matrix A in LDS by one thread: EPI_SWEEPS sweeps over p < q in row-major order; V (N x N) gets the
// eigenvectors as columns, the diagonal of A the eigenvalues.  The pair (p, q) is a runtime index, so the matrices stay in LDS; the two
// lines a rotation mixes are staged through registers (compile-time indices), so their N reads are in flight together instead of one
// LDS round trip per element.
template <int N>
__device__ __forceinline__ void epi_rotate_lds(double* M, int ip, int iq, int stride, double c, double s) {
    double xp[N], xq[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { xp[k] = M[ip + k * stride]; xq[k] = M[iq + k * stride]; }
#pragma unroll
    for (int k = 0; k < N; ++k) { M[ip + k * stride] = c * xp[k] - s * xq[k]; M[iq + k * stride] = s * xp[k] + c * xq[k]; }
}

template <int N>
__device__ __forceinline__ void epi_jacobi_lds(double* A, double* V) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) V[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < EPI_SWEEPS; ++sweep)
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                epi_rotate_lds<N>(A, p, q, N, c, s);          // columns p, q of A
                epi_rotate_lds<N>(A, p * N, q * N, 1, c, s);  // rows p, q of A
                epi_rotate_lds<N>(V, p, q, N, c, s);          // columns p, q of V
            }
}

// index of the smallest diagonal entry (the first on ties); false: the second-smallest is <= 1e-12 x the largest, or an entry is not finite
__device__ __forceinline__ bool epi_smallest(const double* A, int n, bool need_gap, int& idx) {
    int i0 = 0;
    bool fin = true;
    for (int i = 0; i < n; ++i) {
        fin = fin && epi_finite(A[i * n + i]);
        if (A[i * n + i] < A[i0 * n + i0]) i0 = i;
    }
    idx = i0;
    if (!fin) return false;
    if (!need_gap) return true;
    double second = EPI_DBL_MAX, largest = -EPI_DBL_MAX;
    for (int i = 0; i < n; ++i) {
        if (i != i0 && A[i * n + i] < second) second = A[i * n + i];
        if (A[i * n + i] > largest) largest = A[i * n + i];
    }
    return second > 1e-12 * largest;
}
