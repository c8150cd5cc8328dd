// Plane-aware epipolar verification for gfx950 ("plane-and-parallax"): when most matches lie on one plane the 8-point F of
// epipolar.hip is one of a family.  Here the plane's homography H (spatial.hip) is taken as known, every match OFF the plane gives one line
// l = (H x1) x x2 through the epipole of image 2, two such lines give e, and F = [e]x H.  The rules are stated in include/affnet_hip.h.
//
//   (affnet_verify_matches, homography)   H, the plane mask and the plane summary, into the caller's buffers
//   (affnet_epipolar_verify)              the plain F, into the caller's buffers
//   epp_list_kernel    one workgroup: per tentative the centres (spv_gather: indices tested before any load) -> pts[t]; the matches that are
//                      usable and not in the plane mask, compacted in ascending t (ballot + wave totals per 256 rows) -> list[0..U), off[t], U
//   epp_hyp_kernel     one thread per hypothesis (a, r), fp64: partner b by the hash, the two lines, e = la x lb, F = [e]x H -> hyp[h] nine fp32,
//                      counts[h] = 0.  Everything a thread indexes at run time is in global memory, its own numbers are in registers.
//   epp_score_kernel   epi_score_rows of epipolar_dev.h: U x rounds hypotheses against all T matches.
//   epp_select_kernel  spv_select_rows over the U x rounds counts.
//   epp_refit_kernel   one workgroup, fp64: N = sum of l l^T over the inliers off the plane by the fixed-order sums of spv_block_sum, its smallest
//                      eigenvector by the 3 x 3 cyclic Jacobi in LDS, F = [e]x H, new mask; then the decision against the plain result.
#include "epipolar_dev.h"

#define EPP_NSUM 6          // upper triangle of the 3 x 3 matrix N

// un, four int32 of scratch: {U, U as the stages use it (0 when they are skipped), best hypothesis, its count}
struct EppIn {
    SpvIn in;
    const double* plane; const uint8_t* plane_inlier; const int32_t* plane_summary;
};

__device__ __forceinline__ void epp_load_h(const double* __restrict__ plane, double (&H)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = plane[i];
}

// l = (H (x, y, 1)) x (u, v, 1), scaled to l0^2 + l1^2 = 1.  false: that norm is zero or not finite (NaN centres end here too).
__device__ __forceinline__ bool epp_line(const double (&H)[9], const float4 p, double (&l)[3]) {
    const double x = p.x, y = p.y, u = p.z, v = p.w;
    const double p0 = (H[0] * x + H[1] * y) + H[2], p1 = (H[3] * x + H[4] * y) + H[5], p2 = (H[6] * x + H[7] * y) + H[8];
    const double l0 = p1 - p2 * v, l1 = p2 * u - p0, l2 = p0 * v - p1 * u;
    const double n = sqrt(l0 * l0 + l1 * l1);
    if (!(n > 0.0) || !epi_finite(n)) return false;
    l[0] = l0 / n; l[1] = l1 / n; l[2] = l2 / n;
    return true;
}

// F = [e]x H, unit norm, sign rule.  false: the norm is zero or not finite.
__device__ __forceinline__ bool epp_model(const double (&e)[3], const double (&H)[9], double (&F)[9]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        F[c] = e[1] * H[6 + c] - e[2] * H[3 + c];
        F[3 + c] = e[2] * H[c] - e[0] * H[6 + c];
        F[6 + c] = e[0] * H[3 + c] - e[1] * H[c];
    }
    return epi_unit_sign(F);
}

// ---- the off-plane list ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void epp_list_kernel(EppIn a, float4* __restrict__ pts, uint8_t* __restrict__ off, int32_t* __restrict__ list,
                                                       int32_t* __restrict__ un, int32_t* __restrict__ n_off) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = spv_rows(a.in.count, a.in.t_max);
    const float qn = __builtin_nanf("");
    int base = 0;                                              // the same on every thread
    for (int t0 = 0; t0 < rows; t0 += 256) {
        const int t = t0 + tid;
        bool flag = false;
        if (t < rows) {
            float4 p = make_float4(qn, qn, qn, qn);
            float A[6], B[6];
            if (spv_gather(a.in, t, A, B) && spv_centres_finite(A, B)) {
                p = make_float4(A[2], A[5], B[2], B[5]);
                flag = a.plane_inlier[t] == 0;
            }
            pts[t] = p;
            off[t] = flag ? 1 : 0;
        }
        const unsigned long long bal = __ballot(flag);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int o = base;
        for (int w = 0; w < wave; ++w) o += s_w[w];
        if (flag) list[o + before] = t;                        // o + before < rows: at most one entry per row below t
        base += ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
        __syncthreads();
    }
    if (tid == 0) {
        const int used = ((a.plane_summary[3] & 1) || base < 2) ? 0 : base;
        un[0] = base; un[1] = used;
        if (n_off) { n_off[0] = base; n_off[1] = used; }
    }
}

// ---- hypotheses ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EPI_ST) void epp_hyp_kernel(const float4* __restrict__ pts, const int32_t* __restrict__ list, const int32_t* __restrict__ un,
                                                         const double* __restrict__ plane, int rounds, uint32_t seed, float* __restrict__ hyp,
                                                         int32_t* __restrict__ counts) {
    const int U = un[1];
    const long long h64 = (long long)blockIdx.x * EPI_ST + threadIdx.x;
    if (h64 >= (long long)U * rounds) return;
    const int h = (int)h64;
    const uint32_t ia = (uint32_t)(h / rounds), r = (uint32_t)(h % rounds);
    uint32_t ib = (uint32_t)(((uint64_t)epi_member_hash(ia, r, 1u, seed) * (uint32_t)U) >> 32);
    if (ib == ia) ib = (ib + 1) % (uint32_t)U;                 // U >= 2
    double H[9], la[3], lb[3], F[9];
    epp_load_h(plane, H);
    bool ok = epp_line(H, pts[list[ia]], la);
    ok = epp_line(H, pts[list[ib]], lb) && ok;
    if (ok) {
        const double e[3] = {la[1] * lb[2] - la[2] * lb[1], la[2] * lb[0] - la[0] * lb[2], la[0] * lb[1] - la[1] * lb[0]};
        ok = epp_model(e, H, F);
    }
    float* out = hyp + 9 * (size_t)h;
    const float qn = __builtin_nanf("");
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = ok ? (float)F[i] : qn;
    counts[h] = 0;
}

// ---- score + select --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EPI_HT) void epp_score_kernel(const float4* __restrict__ pts, const float* __restrict__ hyp, const int32_t* __restrict__ count,
                                                           int t_max, const int32_t* __restrict__ un, int rounds, float th2, int32_t* __restrict__ counts) {
    epi_score_rows(pts, hyp, spv_rows(count, t_max), (long long)un[1] * rounds, th2, counts, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void epp_select_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ un, int rounds, int32_t* __restrict__ best) {
    spv_select_rows(counts, un[1] * rounds, best);
}

// ---- refit + decision ------------------------------------------------------------------------------------------------------------------
struct EppLo {
    const int32_t* count; int t_max;
    const float4* pts; const uint8_t* off; const float* hyp; const double* plane;
    const int32_t* un;         // {U, U used}
    const int32_t* best;       // {index, count} of epp_select_kernel
    float th; int lo_iters;
    uint8_t* cur; uint8_t* keep;                               // scratch: the current mask, the mask of the kept model
    double* model_out; uint8_t* inlier; int32_t* summary;      // hold the plain result on entry
    int32_t* info;
};

__global__ __launch_bounds__(EPI_LO_THREADS) void epp_refit_kernel(EppLo a) {
    __shared__ double s_part[4 * EPP_NSUM], s_sum[EPP_NSUM];
    __shared__ double s_N[9], s_V[9];
    __shared__ double s_m[2][9];           // 0: the candidate's epipole (three numbers), 1: kept model
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    const int rows = spv_rows(a.count, a.t_max);
    const int best = a.best[0];
    const int n_plain = a.summary[2];      // read by every thread before the barrier in front of the only write
    if (best < 0) {                        // the stages did not run, or no hypothesis is valid: the plain result stays
        if (tid == 0) { a.info[0] = a.un[0]; a.info[1] = -1; a.info[2] = 0; a.info[3] = 0; }
        return;
    }
    double H[9];
    epp_load_h(a.plane, H);
    float Ff[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Ff[i] = a.hyp[9 * (size_t)best + i];
    if (tid < 9) s_m[1][tid] = (double)a.hyp[9 * (size_t)best + tid];      // model 0: the hypothesis itself
    if (tid == 0) s_stop = 0;
    const float th2f = a.th * a.th;
    const double th2 = (double)a.th * (double)a.th;
    int n_best, flags = 0;
    {
        double v[1] = {0.0};
        for (int t = tid; t < rows; t += EPI_LO_THREADS) {
            const bool in = epi_inlier(Ff, a.pts[t], th2f);
            a.cur[t] = in; a.keep[t] = in;             // thread tid owns rows tid, tid + 256, ... of both masks throughout
            v[0] += in ? 1.0 : 0.0;
        }
        spv_block_sum<1>(v, s_part, s_sum);
        n_best = (int)v[0];
    }
    for (int it = 0; it < a.lo_iters; ++it) {
        // S = current mask, off the plane, with a usable line; acc[6] counts it
        double acc[EPP_NSUM + 1];
#pragma unroll
        for (int k = 0; k <= EPP_NSUM; ++k) acc[k] = 0.0;
        for (int t = tid; t < rows; t += EPI_LO_THREADS)
            if (a.cur[t] && a.off[t]) {
                double l[3];
                if (epp_line(H, a.pts[t], l)) {
                    acc[0] += l[0] * l[0]; acc[1] += l[0] * l[1]; acc[2] += l[0] * l[2];
                    acc[3] += l[1] * l[1]; acc[4] += l[1] * l[2]; acc[5] += l[2] * l[2];
                    acc[6] += 1.0;
                }
            }
        {
            double n[1] = {acc[6]};
            spv_block_sum<1>(n, s_part, s_sum);
            if ((int)n[0] < 2) { flags |= 2; break; }
        }
        double sums[EPP_NSUM];
#pragma unroll
        for (int k = 0; k < EPP_NSUM; ++k) sums[k] = acc[k];
        spv_block_sum<EPP_NSUM>(sums, s_part, s_sum);
        if (tid == 0) {
            s_N[0] = sums[0]; s_N[1] = sums[1]; s_N[2] = sums[2];
            s_N[3] = sums[1]; s_N[4] = sums[3]; s_N[5] = sums[4];
            s_N[6] = sums[2]; s_N[7] = sums[4]; s_N[8] = sums[5];
            epi_jacobi_lds<3>(s_N, s_V);
            int e;
            const bool ok = epi_smallest(s_N, 3, true, e);
            s_m[0][0] = s_V[e]; s_m[0][1] = s_V[3 + e]; s_m[0][2] = s_V[6 + e];
            s_stop = ok ? 0 : 1;
        }
        __syncthreads();
        if (s_stop) { flags |= 4; break; }
        const double e[3] = {s_m[0][0], s_m[0][1], s_m[0][2]};
        double F[9];
        if (!epp_model(e, H, F)) { flags |= 4; break; }       // every thread, the same numbers
        double v[1] = {0.0};
        for (int t = tid; t < rows; t += EPI_LO_THREADS) {
            const bool in = epi_inlier64(F, a.pts[t], th2);
            a.cur[t] = in;
            v[0] += in ? 1.0 : 0.0;
        }
        spv_block_sum<1>(v, s_part, s_sum);
        if ((int)v[0] > n_best) {          // strict: on a tie the earliest model stays
            n_best = (int)v[0];
            for (int t = tid; t < rows; t += EPI_LO_THREADS) a.keep[t] = a.cur[t];
            if (tid == 0) {                // every thread holds the same F: one of them stores it, by compile-time indices
#pragma unroll
                for (int i = 0; i < 9; ++i) s_m[1][i] = F[i];
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) { a.info[0] = a.un[0]; a.info[1] = best; a.info[2] = a.best[1]; a.info[3] = n_best; }
    if (n_best > n_plain) {                // strictly more inliers than the plain model: this one is the result
        for (int t = tid; t < rows; t += EPI_LO_THREADS) a.inlier[t] = a.keep[t];
        if (tid < 9) a.model_out[tid] = s_m[1][tid];
        if (tid == 0) { a.summary[0] = best; a.summary[1] = a.best[1]; a.summary[2] = n_best; a.summary[3] = flags | AFFNET_EPI_FLAG_PLANAR; }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// scratch: the scratch of the two calls this one contains (they run one after the other: one area, the larger of the two) |
// plane counts int32 [t_max] | pts float4 [t_max] | list int32 [t_max] | hyp float [9 t_max rounds] | counts int32 [t_max rounds] | un int32 [4] |
// off, cur, keep uint8 [t_max] each; every area padded to 16 bytes
struct EppBuf {
    void* sub; int32_t* plane_counts; float4* pts; int32_t* list; float* hyp; int32_t* counts; int32_t* un; uint8_t* off; uint8_t* cur; uint8_t* keep;
    size_t bytes;
};

static EppBuf epp_carve(void* d_scratch, int t_max, int rounds) {
    const size_t t = t_max > 0 ? (size_t)t_max : 0, r = rounds > 0 ? (size_t)rounds : 0;
    const size_t s_plane = affnet_verify_scratch_bytes(t_max), s_epi = affnet_epipolar_scratch_bytes(t_max, rounds);
    char* p = (char*)d_scratch;
    EppBuf b;
    b.sub = p; p += aff_align(s_plane > s_epi ? s_plane : s_epi, 16);
    b.plane_counts = (int32_t*)p; p += aff_align(t * sizeof(int32_t), 16);
    b.pts = (float4*)p; p += t * sizeof(float4);
    b.list = (int32_t*)p; p += aff_align(t * sizeof(int32_t), 16);
    b.hyp = (float*)p; p += aff_align(9 * t * r * sizeof(float), 16);
    b.counts = (int32_t*)p; p += aff_align(t * r * sizeof(int32_t), 16);
    b.un = (int32_t*)p; p += 16;
    b.off = (uint8_t*)p; p += aff_align(t, 16);
    b.cur = (uint8_t*)p; p += aff_align(t, 16);
    b.keep = (uint8_t*)p; p += aff_align(t, 16);
    b.bytes = (size_t)(p - (char*)d_scratch) + 64;
    return b;
}

extern "C" size_t affnet_epipolar_planar_scratch_bytes(int t_max, int rounds) { return epp_carve(nullptr, t_max, rounds).bytes; }

static int epp_check(affnet_ctx* ctx, const char* what, const void* d_lafs1, int n1, const void* d_lafs2, int n2, const void* d_tent, int t_max, float inl_th,
                     float plane_th, int rounds, int lo_iters, const void* d_counts, const void* d_plane, const void* d_plane_inlier, const void* d_plane_summary,
                     const void* d_scratch) {
    if (!ctx || !d_lafs1 || !d_lafs2 || !d_tent || !d_counts || !d_plane || !d_plane_inlier || !d_plane_summary || !d_scratch || n1 < 0 || n2 < 0 || t_max < 0)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: bad argument", what);
    if (((uintptr_t)d_scratch & 15) != 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: d_scratch must be 16-byte aligned", what);
    if (!(inl_th > 0.0f) || !(fabsf(inl_th) <= 3.402823466e38f)) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: inl_th must be finite and > 0", what);
    if (!(plane_th > 0.0f) || !(fabsf(plane_th) <= 3.402823466e38f)) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: plane_th must be finite and > 0", what);
    if (rounds < 1 || rounds > AFFNET_EPI_MAX_ROUNDS) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: rounds %d outside 1..%d", what, rounds, AFFNET_EPI_MAX_ROUNDS);
    if ((long long)t_max * rounds > 0x7fffffffLL) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: t_max * rounds = %lld hypotheses (at most 2^31 - 1)", what, (long long)t_max * rounds);
    if (lo_iters < 0 || lo_iters > 8) return aff_fail(ctx, AFFNET_ERR_INVALID, "%s: lo_iters %d outside 0..8", what, lo_iters);
    return AFFNET_OK;
}

// stages 3 to 6 behind the plane's outputs: list, hypotheses, score, select
static void epp_score_launch(const EppIn& a, float inl_th, int rounds, uint32_t seed, const EppBuf& b, int32_t* list, int32_t* n_off, float* hyp, int32_t* counts,
                             int32_t* best, hipStream_t st) {
    const int t_max = a.in.t_max;
    hipLaunchKernelGGL(epp_list_kernel, dim3(1), dim3(256), 0, st, a, b.pts, b.off, list, b.un, n_off);
    if (t_max > 0) {
        const int nh = t_max * rounds;
        hipLaunchKernelGGL(epp_hyp_kernel, dim3(aff_cdiv(nh, EPI_ST)), dim3(EPI_ST), 0, st, (const float4*)b.pts, (const int32_t*)list, (const int32_t*)b.un, a.plane,
                           rounds, seed, hyp, counts);
        hipLaunchKernelGGL(epp_score_kernel, dim3(aff_cdiv(nh, EPI_HT), aff_cdiv(t_max, EPI_MC)), dim3(EPI_HT), 0, st, (const float4*)b.pts, (const float*)hyp,
                           a.in.count, t_max, (const int32_t*)b.un, rounds, inl_th * inl_th, counts);
    }
    hipLaunchKernelGGL(epp_select_kernel, dim3(1), dim3(256), 0, st, (const int32_t*)counts, (const int32_t*)b.un, rounds, best);
}

extern "C" int affnet_epipolar_planar_score(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent, const int32_t* d_count,
                                            int t_max, float inl_th, float plane_th, int rounds, uint32_t seed, int lo_iters, double* d_plane,
                                            uint8_t* d_plane_inlier, int32_t* d_plane_summary, int32_t* d_list, int32_t* d_n_off, float* d_hyp, int32_t* d_counts,
                                            int32_t* d_best, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    { int rc = epp_check(ctx, "epipolar_planar_score", d_lafs1, n1, d_lafs2, n2, d_tent, t_max, inl_th, plane_th, rounds, lo_iters, d_counts, d_plane, d_plane_inlier,
                         d_plane_summary, d_scratch); if (rc) return rc; }
    if (!d_list || !d_n_off || !d_best) return aff_fail(ctx, AFFNET_ERR_INVALID, "epipolar_planar_score: bad argument");
    const EppBuf b = epp_carve(d_scratch, t_max, rounds);
    { int rc = affnet_verify_matches(ctx, d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max, plane_th, AFFNET_VERIFY_HOMOGRAPHY, lo_iters, b.plane_counts, d_plane,
                                     d_plane_inlier, d_plane_summary, b.sub, stream); if (rc) return rc; }
    const EppIn a = {{d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max}, d_plane, d_plane_inlier, d_plane_summary};
    epp_score_launch(a, inl_th, rounds, seed, b, d_list, d_n_off, d_hyp ? d_hyp : b.hyp, d_counts, d_best, (hipStream_t)stream);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

extern "C" int affnet_epipolar_verify_planar(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent, const int32_t* d_count,
                                             int t_max, float inl_th, float plane_th, int rounds, uint32_t seed, int lo_iters, int32_t* d_counts, double* d_model,
                                             uint8_t* d_inlier, int32_t* d_summary, double* d_plane, uint8_t* d_plane_inlier, int32_t* d_plane_summary,
                                             int32_t* d_planar_info, void* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    { int rc = epp_check(ctx, "epipolar_verify_planar", d_lafs1, n1, d_lafs2, n2, d_tent, t_max, inl_th, plane_th, rounds, lo_iters, d_counts, d_plane, d_plane_inlier,
                         d_plane_summary, d_scratch); if (rc) return rc; }
    if (!d_model || !d_inlier || !d_summary || !d_planar_info) return aff_fail(ctx, AFFNET_ERR_INVALID, "epipolar_verify_planar: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const EppBuf b = epp_carve(d_scratch, t_max, rounds);
    { int rc = affnet_verify_matches(ctx, d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max, plane_th, AFFNET_VERIFY_HOMOGRAPHY, lo_iters, b.plane_counts, d_plane,
                                     d_plane_inlier, d_plane_summary, b.sub, stream); if (rc) return rc; }
    { int rc = affnet_epipolar_verify(ctx, d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max, inl_th, rounds, seed, lo_iters, d_counts, d_model, d_inlier, d_summary,
                                      b.sub, stream); if (rc) return rc; }
    const EppIn a = {{d_lafs1, n1, d_lafs2, n2, d_tent, d_count, t_max}, d_plane, d_plane_inlier, d_plane_summary};
    epp_score_launch(a, inl_th, rounds, seed, b, b.list, nullptr, b.hyp, b.counts, b.un + 2, st);
    EppLo lo;
    lo.count = d_count; lo.t_max = t_max; lo.pts = b.pts; lo.off = b.off; lo.hyp = b.hyp; lo.plane = d_plane; lo.un = b.un; lo.best = b.un + 2;
    lo.th = inl_th; lo.lo_iters = lo_iters; lo.cur = b.cur; lo.keep = b.keep;
    lo.model_out = d_model; lo.inlier = d_inlier; lo.summary = d_summary; lo.info = d_planar_info;
    hipLaunchKernelGGL(epp_refit_kernel, dim3(1), dim3(EPI_LO_THREADS), 0, st, lo);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}
