// Device functions shared by the verification kernels of matches from affine frames: spatial.hip (planar models) and epipolar.hip
// (fundamental matrix).  What both mean by "the rows of a call", "a usable match" and "the best hypothesis" is written here once.
#pragma once
#include "common.h"

struct SpvIn {
    const float* lafs1; int n1;
    const float* lafs2; int n2;
    const int32_t* tent;
    const int32_t* count;      // device row count or NULL (= t_max rows)
    int t_max;
};

// The arguments that every kernel of a *_many verification shares (affnet_verify_matches_many, affnet_epipolar_verify_many): the two sides, the
// pair table, the pair-major tentative lists and the pair-major scratch that both model families keep.
struct SpvMany {
    const float* lafs1; int rows1;
    const float* lafs2; int rows2;
    const int32_t* pairs;
    const int32_t* tent;       // (P, t_max, 2)
    const int32_t* count;      // (P) or NULL
    int t_max;
    float4* pts; float4* hyp;  // scratch: (P, t_max) each; epipolar.hip keeps the frames in hyp, (P, 3 t_max)
    int32_t* best;             // scratch: (P, 4), {index, count} of the pair in the first two
};

// false: pair row out of range
__device__ __forceinline__ bool spv_many_in(const SpvMany& m, int p, SpvIn& in) {
    AffPairRow r;
    if (!aff_pair_row(m.pairs, p, m.rows1, m.rows2, m.t_max, 0x7fffffff, r)) return false;
    in.lafs1 = m.lafs1 + 6 * (size_t)r.row1; in.n1 = r.n1;
    in.lafs2 = m.lafs2 + 6 * (size_t)r.row2; in.n2 = r.n2;
    in.tent = m.tent + 2 * (size_t)p * m.t_max;
    in.count = m.count ? m.count + p : nullptr;
    in.t_max = m.t_max;
    return true;
}

__device__ __forceinline__ int spv_rows(const int32_t* count, int t_max) {
    if (!count) return t_max;
    return min(max(*count, 0), t_max);
}

__device__ __forceinline__ bool spv_finite(float x) { return fabsf(x) <= 3.402823466e38f; }     // false for NaN and +-inf

// The two frames of tentative t, each as the six floats of its (2,3) row: [a b x; c d y].  false, and nothing loaded, when an index is
// outside its frame list (the bounds guard: such an index never becomes a load).
__device__ __forceinline__ bool spv_gather(const SpvIn& in, int t, float (&A)[6], float (&B)[6]) {
    const int i = in.tent[2 * t], j = in.tent[2 * t + 1];
    if (!(i >= 0 && i < in.n1 && j >= 0 && j < in.n2)) return false;
    const float* pa = in.lafs1 + 6 * (size_t)i;
    const float* pb = in.lafs2 + 6 * (size_t)j;
#pragma unroll
    for (int k = 0; k < 6; ++k) { A[k] = pa[k]; B[k] = pb[k]; }
    return true;
}

// a usable match: both centres finite
__device__ __forceinline__ bool spv_centres_finite(const float (&A)[6], const float (&B)[6]) {
    return spv_finite(A[2]) && spv_finite(A[5]) && spv_finite(B[2]) && spv_finite(B[5]);
}

// a usable hypothesis needs the eight shape numbers finite as well
__device__ __forceinline__ bool spv_shapes_finite(const float (&A)[6], const float (&B)[6]) {
    return spv_finite(A[0]) && spv_finite(A[1]) && spv_finite(A[3]) && spv_finite(A[4]) && spv_finite(B[0]) && spv_finite(B[1]) && spv_finite(B[3]) &&
           spv_finite(B[4]);
}

// best[0] = smallest h in [0, rows) with the largest count, best[1] = that count; {-1, 0} when no hypothesis has an inlier (no valid
// hypothesis, or no rows).  One workgroup of 256 threads.
__device__ __forceinline__ void spv_select_rows(const int32_t* __restrict__ counts, int rows, int32_t* __restrict__ best) {
    __shared__ int s_c[4], s_i[4];
    int bc = 0, bi = 0x7fffffff;
    for (int h = threadIdx.x; h < rows; h += 256) {           // ascending h: the strict > keeps the smallest index
        const int c = counts[h];
        if (c > bc) { bc = c; bi = h; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o, 64), oi = __shfl_xor(bi, o, 64);
        if (oc > bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = bc; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (s_c[w] > bc || (s_c[w] == bc && s_i[w] < bi)) { bc = s_c[w]; bi = s_i[w]; }
        best[0] = bc > 0 ? bi : -1;
        best[1] = bc > 0 ? bc : 0;
    }
}

// v[k] <- sum over a workgroup of 256 threads, the same on every thread.  Fixed order: wave butterfly, then waves 0..3 left to right.
// s_part holds 4 K doubles, s_sum K.
template <int K>
__device__ __forceinline__ void spv_block_sum(double (&v)[K], double* s_part, double* s_sum) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_part[wave * K + k] = v[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < K) s_sum[threadIdx.x] = ((s_part[threadIdx.x] + s_part[K + threadIdx.x]) + s_part[2 * K + threadIdx.x]) + s_part[3 * K + threadIdx.x];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = s_sum[k];
    __syncthreads();
}
