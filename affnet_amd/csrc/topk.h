// The candidate lists of the descriptor index (knn.hip, knn_q8.hip, ivf.hip), device code only: the order of candidates, a sorted list in
// registers and the merge of the lists of neighbouring lanes.  Written once over the distance type D:
// float (the matcher's distance) or int (the int8 path's exact squared distance).
//
// Order of candidates, everywhere: a NaN distance (float only: the fp32 expansion can go below -1e-6 for near-identical vectors) in front of
// every number, then the smaller distance, then the smaller row.  The order is total and every distance is computed once, so a result does not
// depend on how the candidates were cut into lists: not on the number of chunks, not on which lane or wave met a candidate first.
//
// An unfilled slot is (topk_far<D>(), TOPK_EMPTY): behind every real candidate in the order.  What a caller writes out for it (-1, +inf) is the
// caller's business.
//
// The first k of the union of the lists of W lanes are k rounds of topk_lanes_next.  That loop stays with its callers (knn_lanes_store,
// q8_lanes_store, ivf_tile_kernel): they differ in what the writing lane stores per round, and handing the store in as a callable changed the
// instruction schedule of tile kernels; so did a shared helper for the gather at the head of the two merge kernels, for theirs (DESIGN.md,
// descriptor index: what is shared).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define TOPK_EMPTY 0x7fffffff          // row of an unfilled slot

template <typename D> __device__ __forceinline__ D topk_far();
template <> __device__ __forceinline__ float topk_far<float>() { return INFINITY; }
template <> __device__ __forceinline__ int topk_far<int>() { return 0x7fffffff; }

// (d, c) stands in front of (s, si)
__device__ __forceinline__ bool topk_before(float d, int c, float s, int si) {
    const bool dn = d != d, sn = s != s;
    return dn ? (!sn || c < si) : (!sn && (d < s || (d == s && c < si)));
}
__device__ __forceinline__ bool topk_before(int d, int c, int s, int si) { return d < s || (d == s && c < si); }

// A sorted list of CAP candidates in registers (compile-time indices only: a dynamically indexed array would live in scratch memory).
template <typename D, int CAP>
struct TopkList {
    D d[CAP];
    int i[CAP];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < CAP; ++s) { d[s] = topk_far<D>(); i[s] = TOPK_EMPTY; }
    }
    // the candidate replaces the last slot when it stands in front of it, then rises to its place
    __device__ __forceinline__ void insert(D nd, int ni) {
        if (!topk_before(nd, ni, d[CAP - 1], i[CAP - 1])) return;
        d[CAP - 1] = nd; i[CAP - 1] = ni;
#pragma unroll
        for (int s = CAP - 1; s > 0; --s) {
            const bool up = topk_before(d[s], i[s], d[s - 1], i[s - 1]);
            const D td = d[s - 1]; const int ti = i[s - 1];
            d[s - 1] = up ? d[s] : td; i[s - 1] = up ? i[s] : ti;
            d[s] = up ? td : d[s]; i[s] = up ? ti : i[s];
        }
    }
    __device__ __forceinline__ void pop(bool yes) {
#pragma unroll
        for (int s = 0; s + 1 < CAP; ++s) { d[s] = yes ? d[s + 1] : d[s]; i[s] = yes ? i[s + 1] : i[s]; }
        d[CAP - 1] = yes ? topk_far<D>() : d[CAP - 1]; i[CAP - 1] = yes ? TOPK_EMPTY : i[CAP - 1];
    }
};

// One round of the merge of the sorted lists of W neighbouring lanes (W = 16 or 64, a power of two): a butterfly minimum over the lists' heads,
// after which every lane holds the winner (bd, bi), and the lane whose head it was (real rows are unique over the lanes) drops it.
template <int W, typename D, int CAP>
__device__ __forceinline__ void topk_lanes_next(TopkList<D, CAP>& L, D& bd, int& bi) {
    bd = L.d[0];
    bi = L.i[0];
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        const D od = __shfl_xor(bd, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        const bool take = topk_before(od, oi, bd, bi);
        bd = take ? od : bd; bi = take ? oi : bi;
    }
    L.pop(bi != TOPK_EMPTY && L.i[0] == bi);
}

// The distance of the k-th candidate of that union (topk_far while it has fewer than k), on a copy of the lists: nothing behind it can reach a
// row's result (a later candidate of the same distance has a larger row), so the tile loops take it as the row's bound.
template <int W, typename D, int CAP>
__device__ __forceinline__ D topk_lanes_kth(TopkList<D, CAP> L, int k) {
    D kth = topk_far<D>();
    int bi;
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (j < k) topk_lanes_next<W>(L, kth, bi);        // uniform
    return kth;
}
