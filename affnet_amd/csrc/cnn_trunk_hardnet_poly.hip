// The exact HardNet trunk of descriptor form 1 (affnet_set_desc_form): cnn32_trunk_kernel<HardNet, 8, *, 1> (cnn_trunk.h), conv2 / conv4 as polyphase Winograd
// F(2x2, 2x2), and the kernel that derives its weights from the blob.  A unit of its own: the form 0 kernels of cnn_trunk_hardnet.hip share template instances with this
// flow (conv1 / conv3 / conv5), and compiled together the inliner's choices - and with them the form 0 kernels' code - change.
#include "cnn_trunk.h"

// One thread per (cin, cout) pair of conv2 (2048) and conv4 (8192), numbered in the fragment order (so that a wave's loads and stores are contiguous): reads its 9
// BN-folded taps and writes its 25 positions, both in w_tap_index order; the transform and its operation order are poly_weight_transform's (weights_layout.h).
__global__ __launch_bounds__(256) void poly_derive_u_kernel(const float* __restrict__ packed, int w2, int w4, float* __restrict__ U) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Poly32::PAIRS) return;
    const int l = e >= 32 * 64 ? 4 : 2;
    const int cin = 16 * l, cout = 32 * l;                              // 32 -> 64, 64 -> 128
    const float* src = packed + (l == 4 ? w4 : w2);
    float* dst = U + Poly32::offset(l);
    e -= l == 4 ? 32 * 64 : 0;
    const int n = (e >> 2) % cout, c = (e >> 2) / cout * 4 + (e & 3);   // e == w_tap_index(0, c, n, cin, cout)
    float g[9], u[POLY_XI];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = src[w_tap_index(t, c, n, cin, cout)];
    poly_weight_transform(g, u);
#pragma unroll
    for (int xi = 0; xi < POLY_XI; ++xi) dst[w_tap_index(xi, c, n, cin, cout)] = u[xi];
}

// The context's buffer of derived HardNet weights: the polyphase ones (Poly32::FLOATS) and behind them form 2's F(4x4, 3x3) ones (F43::FLOATS at F43::BASE,
// cnn_trunk_hardnet_f43.hip).  Allocated on first use; affnet_graph_capture_extract calls this before the capture begins (no allocation inside a capture).
int aff_poly_u_ensure(affnet_ctx* ctx) {
    if (ctx->poly_u) return AFFNET_OK;
    AFF_HIP(ctx, hipMalloc((void**)&ctx->poly_u, (size_t)(Poly32::FLOATS + F43::FLOATS) * sizeof(float)));
    return AFFNET_OK;
}

// U of conv2 / conv4 of `packed` (HardNet blob) into the context's buffer, on the launch stream: 10240 threads, 0.37 MB read, 1.0 MB written.  In front of EVERY
// form 1 trunk launch, so that a blob rewritten in place can never meet stale weights, eagerly or in a replayed graph.
int aff_poly_derive_u(affnet_ctx* ctx, const float* packed, const NetLayout& L, hipStream_t st, const float** u) {
    const int rc = aff_poly_u_ensure(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(poly_derive_u_kernel, dim3((Poly32::PAIRS + 255) / 256), dim3(256), 0, st, packed, (int)L.w_off[2], (int)L.w_off[4], ctx->poly_u);
    AFF_LAUNCH_CHECK(ctx);
    *u = ctx->poly_u;
    return AFFNET_OK;
}

// [phase stamps]; stamps = dbg_time or a layer dump
TrunkKernel aff_trunk_hardnet_poly(bool stamps) {
    static const TrunkKernel k[2] = {cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, false, 1>, cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, true, 1>};
    return k[stamps];
}
