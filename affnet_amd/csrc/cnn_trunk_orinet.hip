// OriNet's six instantiations of cnn32_trunk_kernel (cnn_trunk.h), and the Winograd weights U = G g G^T that the exact one reads: derived from the
// blob in front of every launch (Wino16, common.h).
#include "cnn_trunk.h"

// One thread per (cin, cout) pair of conv1 (256), conv3 (1024) and conv5 (4096), numbered in the fragment order (so that a wave's loads and stores are contiguous): reads its
// 9 taps and writes its 16 transform positions, both in w_tap_index order; the transform and its operation order are wino_weight_transform's (weights_layout.h).
// Behind them one thread per (cin, cout) pair of the stride-2 layers conv2 (512) and conv4 (2048): its 9 taps into the 25 polyphase positions of poly_weight_transform
// (weights_layout.h), as poly_derive_u_kernel does for HardNet.
static_assert(POLY_XI * 16 * 32 == Wino16::P2 && POLY_XI * 32 * 64 == Wino16::P4, "Wino16's polyphase sections hold POLY_XI positions");
__global__ __launch_bounds__(256) void wino_derive_u_kernel(const float* __restrict__ packed, int w1, int w3, int w5, int w2, int w4, float* __restrict__ U) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Wino16::PAIRS + Wino16::PAIRS_POLY) return;
    if (e >= Wino16::PAIRS) {
        e -= Wino16::PAIRS;
        const int l = e >= 16 * 32 ? 4 : 2;
        const int cin = 8 * l, cout = 16 * l;                               // 16 -> 32, 32 -> 64
        const float* src = packed + (l == 4 ? w4 : w2);
        float* dst = U + Wino16::offset(l);
        e -= l == 4 ? 16 * 32 : 0;
        const int n = (e >> 2) % cout, c = (e >> 2) / cout * 4 + (e & 3);   // e == w_tap_index(0, c, n, cin, cout)
        float g[9], u[POLY_XI];
#pragma unroll
        for (int t = 0; t < 9; ++t) g[t] = src[w_tap_index(t, c, n, cin, cout)];
        poly_weight_transform(g, u);
#pragma unroll
        for (int xi = 0; xi < POLY_XI; ++xi) dst[w_tap_index(xi, c, n, cin, cout)] = u[xi];
        return;
    }
    const int l = e >= 256 + 1024 ? 5 : (e >= 256 ? 3 : 1);
    const int ch = 8 << ((l + 1) >> 1);                                 // cin == cout: 16, 32, 64
    const float* src = packed + (l == 5 ? w5 : (l == 3 ? w3 : w1));
    float* dst = U + Wino16::offset(l);
    e -= l == 5 ? 256 + 1024 : (l == 3 ? 256 : 0);
    const int n = (e >> 2) % ch, c = (e >> 2) / ch * 4 + (e & 3);       // e == w_tap_index(0, c, n, ch, ch)
    float g[9], u[16];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = src[w_tap_index(t, c, n, ch, ch)];
    wino_weight_transform(g, u);
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) dst[w_tap_index(xi, c, n, ch, ch)] = u[xi];
}

// The context's buffer of derived Winograd weights (Wino16::FLOATS per 16-channel net).  Allocated on first use; affnet_graph_capture_extract calls this
// before the capture begins (no allocation inside a capture).
int aff_wino_u_ensure(affnet_ctx* ctx) {
    if (ctx->wino_u) return AFFNET_OK;
    AFF_HIP(ctx, hipMalloc((void**)&ctx->wino_u, (size_t)2 * Wino16::FLOATS * sizeof(float)));
    return AFFNET_OK;
}

// U of conv1 / conv3 / conv5 and the polyphase positions of conv2 / conv4 of `packed` (AffNet or OriNet blob) into the context's region of that net, on the launch stream:
// 7936 threads, 286 KB read, 600 KB written.
// In front of EVERY exact OriNet trunk launch, so that a blob rewritten in place (load_state_dict into the same device buffer) can never meet
// stale weights, eagerly or in a replayed graph.
int aff_wino_derive_u(affnet_ctx* ctx, int kind, const float* packed, const NetLayout& L, hipStream_t st, const float** u) {
    const int rc = aff_wino_u_ensure(ctx);
    if (rc) return rc;
    float* dst = ctx->wino_u + (size_t)kind * Wino16::FLOATS;
    hipLaunchKernelGGL(wino_derive_u_kernel, dim3((Wino16::PAIRS + Wino16::PAIRS_POLY + 255) / 256), dim3(256), 0, st, packed, (int)L.w_off[1], (int)L.w_off[3], (int)L.w_off[5],
                       (int)L.w_off[2], (int)L.w_off[4], dst);
    AFF_LAUNCH_CHECK(ctx);
    *u = dst;
    return AFFNET_OK;
}

// [exact, three bf16 terms, two fp16 terms][phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check)
TrunkKernel aff_trunk_orinet(int arith_index, bool stamps) {
    static const TrunkKernel k[3][2] = {{cnn32_trunk_kernel<AFFNET_NET_ORINET, 8, false>, cnn32_trunk_kernel<AFFNET_NET_ORINET, 8, true>},
                                        {cnn32_trunk_kernel<AFFNET_NET_ORINET, 8, false, 3>, cnn32_trunk_kernel<AFFNET_NET_ORINET, 8, true, 3>},
                                        {cnn32_trunk_kernel<AFFNET_NET_ORINET, 8, false, 2>, cnn32_trunk_kernel<AFFNET_NET_ORINET, 8, true, 2>}};
    return k[arith_index][stamps];
}
