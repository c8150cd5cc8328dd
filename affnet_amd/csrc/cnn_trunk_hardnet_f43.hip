// The exact HardNet trunk of descriptor form 2 (affnet_set_desc_form): cnn32_trunk_kernel<HardNet, 8, *, 4> (cnn_trunk.h) = form 1 with conv3 as Winograd
// F(4x4, 3x3), and the kernel that derives that form's weights from the blob.  A unit of its own for the reason cnn_trunk_hardnet_poly.hip is one: compiled beside
// the kernels it shares template instances with (conv0 .. conv2, conv4, conv5), the inliner's choices - and with them those kernels' code - change.
#include "cnn_trunk.h"

// One thread per (cin, cout) pair of conv1 (1024) and conv3 (4096), numbered in the fragment order (so that a wave's loads and stores are contiguous): reads its 9
// BN-folded taps and writes its 36 positions, both in w_tap_index order; the transform and its operation order are f43_weight_transform's (weights_layout.h).
__global__ __launch_bounds__(256) void f43_derive_u_kernel(const float* __restrict__ packed, int w1, int w3, float* __restrict__ U) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= F43::PAIRS) return;
    const int l = e >= 32 * 32 ? 3 : 1;
    const int cin = l == 3 ? 64 : 32, cout = cin;                       // 32 -> 32, 64 -> 64
    const float* src = packed + (l == 3 ? w3 : w1);
    float* dst = U + F43::offset(l);
    e -= l == 3 ? 32 * 32 : 0;
    const int n = (e >> 2) % cout, c = (e >> 2) / cout * 4 + (e & 3);   // e == w_tap_index(0, c, n, cin, cout)
    float g[9], u[F43_XI];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = src[w_tap_index(t, c, n, cin, cout)];
    f43_weight_transform(g, u);
#pragma unroll
    for (int xi = 0; xi < F43_XI; ++xi) dst[w_tap_index(xi, c, n, cin, cout)] = u[xi];
}

// U of conv1 / conv3 of `packed` (HardNet blob) behind the polyphase weights in the context's buffer (aff_poly_u_ensure allocates both families), on the launch stream:
// 5120 threads, 0.18 MB read, 0.74 MB written.  In front of EVERY form 2 trunk launch, next to aff_poly_derive_u and for its reason: a blob rewritten in place can
// never meet stale weights, eagerly or in a replayed graph.
int aff_f43_derive_u(affnet_ctx* ctx, const float* packed, const NetLayout& L, hipStream_t st) {
    const int rc = aff_poly_u_ensure(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(f43_derive_u_kernel, dim3((F43::PAIRS + 255) / 256), dim3(256), 0, st, packed, (int)L.w_off[1], (int)L.w_off[3], ctx->poly_u + F43::BASE);
    AFF_LAUNCH_CHECK(ctx);
    return AFFNET_OK;
}

// [phase stamps]; stamps = dbg_time or a layer dump
TrunkKernel aff_trunk_hardnet_f43(bool stamps) {
    static const TrunkKernel k[2] = {cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, false, 4>, cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, true, 4>};
    return k[stamps];
}
