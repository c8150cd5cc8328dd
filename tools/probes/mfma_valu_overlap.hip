// Does VALU work hide under MFMAs on gfx950?  One workgroup per CU, W waves per SIMD; every wave runs ITER x { NM MFMAs on 4
// independent accumulators, NV VALU instructions of one kind on independent registers }.  Prints cycles per iteration (s_memtime is
// not used: wall clock via hipEvents and the measured shader clock are enough for ratios).
// Two regimes: bf16 MFMAs (8 pipe cycles each, probe<>) and the fp32 MFMA of the exact trunks (v_mfma_f32_16x16x4_f32, 32 pipe cycles,
// probe_f32<>: one step of the paired Winograd row loop = 32 MFMAs on 8 accumulators, 8 ds_read_b128, 32 scalar f32 adds on what they return;
// probe_f43<>: the ratio an F(4x4, 3x3) conv1 with its transform in the loop would have = 24 MFMAs on 6 accumulators, 24 ds_read_b128, 96 scalar f32 adds / fmas,
// 4 VALU per MFMA where the pair loop has 1).
//   hipcc --offload-arch=gfx950 -O3 -o mfma_valu_overlap mfma_valu_overlap.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int NM, int NV, int KIND>
__global__ __launch_bounds__(512) void probe(float* out, int iters) {
    f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    bf16x8 a, b;
    for (int k = 0; k < 8; ++k) { a[k] = (__bf16)(threadIdx.x * 0.001f + k); b[k] = (__bf16)(1.0f + k * 0.01f); }
    float v[8];
    for (int k = 0; k < 8; ++k) v[k] = threadIdx.x * 0.37f + k;
    unsigned c0;
    asm volatile("s_mov_b32 %0, 0xbf80" : "=s"(c0));
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            acc[m & 3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[m & 3], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < NV / (NM > 0 ? NM : 1); ++q) {
                const int r = (m * (NV / (NM > 0 ? NM : 1)) + q) & 7;
                if (KIND == 0) asm volatile("v_fmac_f32 %0, %0, %0" : "+v"(v[r]));
                if (KIND == 1) asm volatile("v_cvt_pk_bf16_f32 %0, %0, %0" : "+v"(v[r]));
                if (KIND == 2) asm volatile("v_dot2c_f32_bf16 %0, %1, %0" : "+v"(v[r]) : "s"(c0));
                if (KIND == 3) asm volatile("v_pk_add_f32 %0, %0, %0" : "+v"(*(f32x2*)&v[r & 6]));
                if (KIND == 4) asm volatile("v_lshlrev_b32 %0, 16, %0" : "+v"(v[r]));
            }
        }
        if (NM == 0) {
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int r = q & 7;
                if (KIND == 0) asm volatile("v_fmac_f32 %0, %0, %0" : "+v"(v[r]));
                if (KIND == 1) asm volatile("v_cvt_pk_bf16_f32 %0, %0, %0" : "+v"(v[r]));
                if (KIND == 2) asm volatile("v_dot2c_f32_bf16 %0, %1, %0" : "+v"(v[r]) : "s"(c0));
                if (KIND == 3) asm volatile("v_pk_add_f32 %0, %0, %0" : "+v"(*(f32x2*)&v[r & 6]));
                if (KIND == 4) asm volatile("v_lshlrev_b32 %0, 16, %0" : "+v"(v[r]));
            }
        }
    }
    float s = 0;
    for (int k = 0; k < 4; ++k) s += acc[k].x + acc[k].y + acc[k].z + acc[k].w;
    for (int k = 0; k < 8; ++k) s += v[k];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// fp32 case.  MODE 0: the 32 MFMAs alone; 1: the 8 reads + 32 adds alone; 2: reads + adds as a block in front of the MFMAs; 3: interleaved 1 : 1,
// add j behind MFMA j on the rows the PREVIOUS iteration requested (two row sets), read j behind MFMA j < 8; 4: as one row set allows: the reads behind
// MFMAs 0..7, the adds two per MFMA behind MFMAs 16..31.
typedef __attribute__((address_space(3))) const f32x4 LdsF4;
template <int MODE>
__global__ __launch_bounds__(512) void probe_f32(float* out, int iters) {
    __shared__ __attribute__((aligned(16))) float lds[8 * 512 * 4 / 2];      // 16 KB: 8 rows of 1 KB per wave pair
    for (int i = threadIdx.x; i < 8 * 512 * 2; i += blockDim.x) lds[i] = 0.001f * (float)(i & 255);
    __syncthreads();
    f32x4 acc[8];
    for (int k = 0; k < 8; ++k) acc[k] = (f32x4){0, 0, 0, 0};
    float a[4], b[4], v[32];
    for (int k = 0; k < 4; ++k) { a[k] = threadIdx.x * 0.001f + k; b[k] = 1.0f + k * 0.01f; }
    for (int k = 0; k < 32; ++k) v[k] = threadIdx.x * 0.37f + k;
    f32x4 d0[8], d1[8];
    for (int k = 0; k < 8; ++k) { d0[k] = (f32x4){1, 2, 3, 4}; d1[k] = d0[k]; }
    unsigned ab = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)lds + (threadIdx.x & 255) * 16;
    auto mfma = [&](int m) {
        acc[(m >> 3) * 2 + (m & 1)] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(m >> 1) & 3], b[(m >> 1) & 3], acc[(m >> 3) * 2 + (m & 1)], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto read = [&](f32x4 (&d)[8], int j) { d[j] = *(LdsF4*)(size_t)(ab + j * 4096); __builtin_amdgcn_sched_barrier(0); };
    auto add = [&](const f32x4 (&d)[8], int j) { asm volatile("v_add_f32 %0, %0, %1" : "+v"(v[j]) : "v"(d[j >> 2][j & 3])); __builtin_amdgcn_sched_barrier(0); };
    auto step = [&](f32x4 (&dc)[8], f32x4 (&dn)[8]) {      // dc: rows in hand, dn: rows requested now (MODE 3 only keeps two sets)
        asm volatile("" : "+v"(ab));
        if (MODE == 1 || MODE == 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) read(dc, j);
#pragma unroll
            for (int j = 0; j < 32; ++j) add(dc, j);
        }
        if (MODE == 1) return;
#pragma unroll
        for (int m = 0; m < 32; ++m) {
            mfma(m);
            if (MODE == 3) { if (m < 8) read(dn, m); add(dc, m); }
            if (MODE == 4) { if (m < 8) read(dc, m); if (m >= 16) { add(dc, 2 * (m - 16)); add(dc, 2 * (m - 16) + 1); } }
        }
    };
    for (int it = 0; it < iters; it += 2) { step(d0, d1); step(d1, d0); }
    float s = 0;
    for (int k = 0; k < 8; ++k) s += acc[k].x + acc[k].y + acc[k].z + acc[k].w;
    for (int k = 0; k < 32; ++k) s += v[k];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// F(4x4, 3x3) ratio.  MODE 0: the 24 MFMAs alone; 1: the 24 reads + 96 VALU alone; 2: reads + VALU as a block in front of the MFMAs; 3: interleaved, behind MFMA j
// read j into the row set of the NEXT iteration and four VALU (two v_add_f32, two v_fma_f32) on the rows the PREVIOUS iteration requested.
template <int MODE>
__global__ __launch_bounds__(512) void probe_f43(float* out, int iters) {
    __shared__ __attribute__((aligned(16))) float lds[24 * 256 * 4];          // 24 KB: 24 rows of 1 KB per wave quad
    for (int i = threadIdx.x; i < 24 * 256 * 4; i += blockDim.x) lds[i] = 0.001f * (float)(i & 255);
    __syncthreads();
    f32x4 acc[6];
    for (int k = 0; k < 6; ++k) acc[k] = (f32x4){0, 0, 0, 0};
    float a[4], b[4], v[32];
    for (int k = 0; k < 4; ++k) { a[k] = threadIdx.x * 0.001f + k; b[k] = 1.0f + k * 0.01f; }
    for (int k = 0; k < 32; ++k) v[k] = threadIdx.x * 0.37f + k;
    f32x4 d0[24], d1[24];
    for (int k = 0; k < 24; ++k) { d0[k] = (f32x4){1, 2, 3, 4}; d1[k] = d0[k]; }
    unsigned ab = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)lds + (threadIdx.x & 255) * 16;
    auto mfma = [&](int m) {
        acc[m % 6] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(m / 6) & 3], b[(m / 6) & 3], acc[m % 6], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto read = [&](f32x4 (&d)[24], int j) { d[j] = *(LdsF4*)(size_t)(ab + j * 4096); __builtin_amdgcn_sched_barrier(0); };
    auto valu = [&](const f32x4 (&d)[24], int j) {        // VALU operation j of 96: operand = element j of the 24 x 4 floats read
        if (j & 1) asm volatile("v_fma_f32 %0, %1, 4.0, %0" : "+v"(v[j & 31]) : "v"(d[j >> 2][j & 3]));
        else asm volatile("v_add_f32 %0, %0, %1" : "+v"(v[j & 31]) : "v"(d[j >> 2][j & 3]));
        __builtin_amdgcn_sched_barrier(0);
    };
    auto step = [&](f32x4 (&dc)[24], f32x4 (&dn)[24]) {
        asm volatile("" : "+v"(ab));
        if (MODE == 1 || MODE == 2) {
#pragma unroll
            for (int j = 0; j < 24; ++j) read(dc, j);
#pragma unroll
            for (int j = 0; j < 96; ++j) valu(dc, j);
        }
        if (MODE == 1) return;
#pragma unroll
        for (int m = 0; m < 24; ++m) {
            mfma(m);
            if (MODE == 3) {
                read(dn, m);
#pragma unroll
                for (int q = 0; q < 4; ++q) valu(dc, 4 * m + q);
            }
        }
    };
    for (int it = 0; it < iters; it += 2) { step(d0, d1); step(d1, d0); }
    float s = 0;
    for (int k = 0; k < 6; ++k) s += acc[k].x + acc[k].y + acc[k].z + acc[k].w;
    for (int k = 0; k < 32; ++k) s += v[k];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int MODE>
static double run_f43(int waves_per_simd, float* d, const char* name) {
    const int iters = 20000, threads = 64 * 4 * waves_per_simd;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    probe_f43<MODE><<<256, threads>>>(d, 100);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    probe_f43<MODE><<<256, threads>>>(d, iters);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double ns_it = ms * 1e6 / iters;
    printf("%-58s waves/SIMD %d: %7.1f ns / iteration  (%6.1f cycles @2.4 GHz)\n", name, waves_per_simd, ns_it, ns_it * 2.4);
    return ns_it;
}

template <int MODE>
static double run_f32(int waves_per_simd, float* d, const char* name) {
    const int iters = 20000, threads = 64 * 4 * waves_per_simd;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    probe_f32<MODE><<<256, threads>>>(d, 100);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    probe_f32<MODE><<<256, threads>>>(d, iters);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double ns_it = ms * 1e6 / iters;
    printf("%-58s waves/SIMD %d: %7.1f ns / iteration  (%6.1f cycles @2.4 GHz)\n", name, waves_per_simd, ns_it, ns_it * 2.4);
    return ns_it;
}

template <int NM, int NV, int KIND>
static double run(int waves_per_simd, float* d, const char* name) {
    const int iters = 20000, threads = 64 * 4 * waves_per_simd;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    probe<NM, NV, KIND><<<256, threads>>>(d, 100);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    probe<NM, NV, KIND><<<256, threads>>>(d, iters);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double ns_it = ms * 1e6 / iters;
    printf("%-34s waves/SIMD %d: %7.1f ns / iteration  (%5.1f cycles @2.4 GHz)\n", name, waves_per_simd, ns_it, ns_it * 2.4);
    return ns_it;
}

int main() {
    float* d;
    (void)hipMalloc(&d, 256 * 512 * 4);
    if (getenv("OVERLAP_F32_ONLY") == nullptr || atoi(getenv("OVERLAP_F32_ONLY")) == 0)
    for (int w = 1; w <= 2; ++w) {
        run<12, 0, 0>(w, d, "12 MFMA");
        run<0, 36, 0>(w, d, "36 v_fmac_f32");
        run<12, 36, 0>(w, d, "12 MFMA + 36 v_fmac_f32");
        run<0, 36, 1>(w, d, "36 v_cvt_pk_bf16_f32");
        run<12, 36, 1>(w, d, "12 MFMA + 36 v_cvt_pk_bf16_f32");
        run<0, 36, 2>(w, d, "36 v_dot2c_f32_bf16");
        run<12, 36, 2>(w, d, "12 MFMA + 36 v_dot2c_f32_bf16");
        run<0, 36, 3>(w, d, "36 v_pk_add_f32");
        run<12, 36, 3>(w, d, "12 MFMA + 36 v_pk_add_f32");
        run<0, 36, 4>(w, d, "36 v_lshlrev_b32");
        run<12, 36, 4>(w, d, "12 MFMA + 36 v_lshlrev_b32");
        run<12, 12, 1>(w, d, "12 MFMA + 12 v_cvt_pk_bf16_f32");
        run<12, 24, 2>(w, d, "12 MFMA + 24 v_dot2c_f32_bf16");
    }
    for (int w = 1; w <= 2; ++w) {
        const double m = run_f32<0>(w, d, "32 fp32 MFMA");
        const double v = run_f32<1>(w, d, "8 ds_read_b128 + 32 v_add_f32");
        const double blk = run_f32<2>(w, d, "(a) reads + adds in a block, then 32 fp32 MFMA");
        const double il = run_f32<3>(w, d, "(b) 32 fp32 MFMA, adds 1 : 1, two row sets");
        const double il1 = run_f32<4>(w, d, "(b') 32 fp32 MFMA, reads early, adds 2 : 1 late, one row set");
        printf("waves/SIMD %d: (a) - (b) = %.1f ns = %.0f %% of the VALU-only time; (a) - (b') = %.1f ns = %.0f %%; (a) - MFMA-only = %.1f ns\n", w, blk - il,
               100.0 * (blk - il) / v, blk - il1, 100.0 * (blk - il1) / v, blk - m);
    }
    for (int w = 1; w <= 2; ++w) {
        const double m = run_f43<0>(w, d, "24 fp32 MFMA");
        const double v = run_f43<1>(w, d, "24 ds_read_b128 + 96 v_add_f32 / v_fma_f32");
        const double blk = run_f43<2>(w, d, "(a) reads + VALU in a block, then 24 fp32 MFMA");
        const double il = run_f43<3>(w, d, "(b) 24 fp32 MFMA, one read and four VALU behind each");
        printf("F(4x4, 3x3) ratio, waves/SIMD %d: (a) - (b) = %.1f ns = %.0f %% of the VALU-only time; (b) - MFMA-only = %.1f ns = %.0f %% of the MFMA-only time\n", w,
               blk - il, 100.0 * (blk - il) / v, il - m, 100.0 * (il - m) / m);
    }
    return 0;
}
