// Counter-calibration kernels, the shape-pass read-back and the Winograd AffNet layer dump of the tests (include/affnet_hip_probes.h): known-byte-count streaming reads / writes / tile loads, so
// that rocprofv3's FETCH_SIZE / WRITE_SIZE can be turned into bytes for the access widths this library actually uses
// (MI355X_MICROARCH.md, HBM section: only 16 B/lane streaming reads are calibrated there).  libaffnet_hip_probes.so only, not part of the product path.
#include "common.h"

#include "../../include/affnet_hip_probes.h"

template <typename T>
__global__ __launch_bounds__(256) void stream_read_kernel(const T* __restrict__ src, float* __restrict__ dst, size_t n_items) {
    // grid-stride, fully coalesced: lane i of a wave reads item base + i
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (size_t)gridDim.x * 256) {
        const T v = src[i];
        const float* f = reinterpret_cast<const float*>(&v);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(T) / 4); ++k) acc += f[k];
    }
    if (acc == 123.456f) dst[blockIdx.x] = acc;       // never true for the calibration pattern: keeps the loads alive
    if (threadIdx.x == 0 && blockIdx.x == 0) dst[0] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void stream_write_kernel(T* __restrict__ dst, size_t n_items) {
    T v;
    float* f = reinterpret_cast<float*>(&v);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) f[k] = (float)(threadIdx.x + k);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (size_t)gridDim.x * 256) dst[i] = v;
}

// 64 x 64 output tile + `halo` apron loaded with 4-byte loads (one float per thread per load), the access pattern of
// blur2d_kernel / hessian_nms_kernel's tile loaders.
__global__ __launch_bounds__(256) void tile_read_kernel(const float* __restrict__ img, float* __restrict__ dst, int h, int w, int halo) {
    const int LW = 64 + 2 * halo, n_el = LW * LW;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n_el; i += 256) {
        const int ty = i / LW, tx = i - ty * LW;
        int gy = y0 + ty - halo, gx = x0 + tx - halo;
        gy = gy < 0 ? 0 : (gy >= h ? h - 1 : gy);
        gx = gx < 0 ? 0 : (gx >= w ? w - 1 : gx);
        acc += img[(size_t)gy * w + gx];
    }
    if (acc == 123.456f) dst[blockIdx.x] = acc;
}

struct f32x2s { float a, b; };

extern "C" int affnet_debug_stream(const void* d_src, void* d_dst, size_t n_bytes, int width, int mode, int halo, void* stream) {
    if (!d_dst || n_bytes == 0 || (n_bytes & 65535) != 0) return AFFNET_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = 256 * 16;     // 16 workgroups per CU
    if (mode == 0) {
        if (!d_src) return AFFNET_ERR_INVALID;
        if (width == 4) hipLaunchKernelGGL(stream_read_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)d_src, (float*)d_dst, n_bytes / 4);
        else if (width == 8) hipLaunchKernelGGL(stream_read_kernel<f32x2s>, dim3(blocks), dim3(256), 0, st, (const f32x2s*)d_src, (float*)d_dst, n_bytes / 8);
        else if (width == 16) hipLaunchKernelGGL(stream_read_kernel<float4>, dim3(blocks), dim3(256), 0, st, (const float4*)d_src, (float*)d_dst, n_bytes / 16);
        else return AFFNET_ERR_INVALID;
    } else if (mode == 1) {
        if (width == 4) hipLaunchKernelGGL(stream_write_kernel<float>, dim3(blocks), dim3(256), 0, st, (float*)d_dst, n_bytes / 4);
        else if (width == 8) hipLaunchKernelGGL(stream_write_kernel<f32x2s>, dim3(blocks), dim3(256), 0, st, (f32x2s*)d_dst, n_bytes / 8);
        else if (width == 16) hipLaunchKernelGGL(stream_write_kernel<float4>, dim3(blocks), dim3(256), 0, st, (float4*)d_dst, n_bytes / 16);
        else return AFFNET_ERR_INVALID;
    } else if (mode == 2) {
        if (!d_src || halo < 0 || halo > 16) return AFFNET_ERR_INVALID;
        const int w = 4096, h = (int)(n_bytes / 4 / w);
        hipLaunchKernelGGL(tile_read_kernel, dim3(w / 64, (h + 63) / 64), dim3(256), 0, st, (const float*)d_src, (float*)d_dst, h, w, halo);
    } else {
        return AFFNET_ERR_INVALID;
    }
    return hipGetLastError() == hipSuccess ? AFFNET_OK : AFFNET_ERR_HIP;
}

extern "C" int affnet_probe_shape_offsets(const affnet_ctx* ctx, int64_t out[3]) {
    if (!ctx || !ctx->ws || !out) return AFFNET_ERR_INVALID;
    out[0] = (int64_t)(reinterpret_cast<const char*>(ctx->st_A) - ctx->ws) / 4;
    // cnn32.hip, cnn_launch: the flags lie behind the head partials of all candidates in the CNN scratch
    out[1] = (int64_t)(reinterpret_cast<const char*>(ctx->st_hard_scratch) - ctx->ws) / 4 + (int64_t)ctx->B * ctx->cap_pre * HEAD_PART_AFF;
    out[2] = (int64_t)(reinterpret_cast<const char*>(ctx->st_det_lafs) - ctx->ws) / 4;
    return AFFNET_OK;
}

// The ledger of the workspace: the table affnet_ctx_create and affnet_bind_workspace carve it from (context.hip: aff_ws_layout), record by record
extern "C" int affnet_probe_workspace_areas(const affnet_ctx* ctx, int max, affnet_ws_area* out) {
    if (!ctx || ctx->ws_bytes == 0 || max < 0 || (max > 0 && !out)) return AFFNET_ERR_INVALID;
    static_assert(AFF_WS_F32 == AFFNET_WS_F32 && AFF_WS_I32 == AFFNET_WS_I32 && AFF_WS_U8 == AFFNET_WS_U8 && AFF_WS_RECORDS == AFFNET_WS_RECORDS &&
                  AFF_WS_GROUP == AFFNET_WS_GROUP, "kinds of the ledger");
    AffWsArea ar[AFF_WS_MAX_AREAS];
    const int n = aff_ws_layout(ctx, ar);
    if (n < 0) return AFFNET_ERR_INVALID;
    for (int i = 0; i < n && i < max; ++i) {
        memset(&out[i], 0, sizeof(out[i]));
        strncpy(out[i].name, ar[i].name, sizeof(out[i].name) - 1);
        out[i].offset = (int64_t)ar[i].off; out[i].bytes = (int64_t)ar[i].bytes;
        out[i].kind = ar[i].kind; out[i].cleared = ar[i].cleared; out[i].parent = ar[i].parent;
    }
    return n;
}

// The Winograd AffNet trunk (the first trunk of shape form 1) on a patch tensor, which no entry point of the product library runs: cnn32.hip's trunk launch (U derived in
// front of it; the stamped instantiation when a layer dump is asked for or the context has a stamp buffer, affnet_cnn32_debug_timing) without a finish stage.
// poly: the first trunk of shape form 2 (conv2 / conv4 polyphase) instead.
static int probe_affnet_wino(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, int layer, hipStream_t st, bool poly = false) {
    if (ctx->arith != AFFNET_ARITH_FP32_MFMA) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_affnet_wino: AFFNET_ARITH_FP32_MFMA only");
    CnnCall c;
    c.kind = AFFNET_NET_AFFNET; c.packed = d_packed; c.patches = d_patches; c.n_max = n; c.st = st;
    c.out = d_out; c.scratch = d_out;                    // a layer dump or the head partials
    c.dbg_layer = layer; c.dbg_out = d_out;
    return aff_trunk_launch(ctx, c, net_layout(AFFNET_NET_AFFNET), dim3(n, 1), poly ? 2 : 1, nullptr, 0);
}

extern "C" int affnet_probe_affnet_wino_layer(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patch || !d_out || net_kind != AFFNET_NET_AFFNET || layer < 0 || layer > 5)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_affnet_wino_layer: AffNet, layer 0 .. 5");
    return probe_affnet_wino(ctx, d_packed, d_patch, 1, d_out, layer, (hipStream_t)stream);
}

extern "C" int affnet_probe_affnet_wino_partials(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_partials, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patches || !d_partials || n < 1 || n > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_affnet_wino_partials: bad argument");
    return probe_affnet_wino(ctx, d_packed, d_patches, n, d_partials, -1, (hipStream_t)stream);
}

extern "C" int affnet_probe_affnet_poly_layer(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patch || !d_out || net_kind != AFFNET_NET_AFFNET || layer < 0 || layer > 5)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_affnet_poly_layer: AffNet, layer 0 .. 5");
    return probe_affnet_wino(ctx, d_packed, d_patch, 1, d_out, layer, (hipStream_t)stream, true);
}

extern "C" int affnet_probe_affnet_poly_partials(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_partials, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patches || !d_partials || n < 1 || n > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_affnet_poly_partials: bad argument");
    return probe_affnet_wino(ctx, d_packed, d_patches, n, d_partials, -1, (hipStream_t)stream, true);
}

// `floats` derived weights at `offset` of the region that trunk form `form` of net `kind` reads, derived from d_packed on the stream and copied to d_out
static int probe_derived_u(affnet_ctx* ctx, int kind, int form, const float* d_packed, int offset, int floats, float* d_out, void* stream) {
    const float* u;
    const int rc = aff_derive_u(ctx, kind, form, d_packed, net_layout(kind), (hipStream_t)stream, &u);
    if (rc) return rc;
    return aff_copy_async(ctx, d_out, u + offset, (size_t)floats * sizeof(float), (hipStream_t)stream);
}

extern "C" int affnet_probe_trunk16_poly_u(affnet_ctx* ctx, int net_kind, const float* d_packed, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_out || (net_kind != AFFNET_NET_AFFNET && net_kind != AFFNET_NET_ORINET) || (layer != 2 && layer != 4))
        return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_trunk16_poly_u: AffNet / OriNet, layer 2 or 4");
    return probe_derived_u(ctx, net_kind, net_kind == AFFNET_NET_AFFNET ? TRUNK_WINO_POLY : TRUNK_EXACT, d_packed, Wino16::offset(layer), Wino16::floats(layer), d_out, stream);
}

extern "C" int affnet_probe_hardnet_poly_layer(affnet_ctx* ctx, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patch || !d_out || layer < 0 || layer > 5) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_poly_layer: layer 0 .. 5");
    return aff_hardnet_poly_patches(ctx, d_packed, d_patch, 1, d_out, nullptr, layer, (hipStream_t)stream);
}

extern "C" int affnet_probe_hardnet_poly_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patches || !d_out || !d_scratch || n < 1 || n > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_poly_forward: bad argument");
    return aff_hardnet_poly_patches(ctx, d_packed, d_patches, n, d_out, d_scratch, -1, (hipStream_t)stream);
}

extern "C" int affnet_probe_hardnet_poly_u(affnet_ctx* ctx, const float* d_packed, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_out || (layer != 2 && layer != 4)) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_poly_u: layer 2 or 4");
    return probe_derived_u(ctx, AFFNET_NET_HARDNET, TRUNK_WINO, d_packed, Poly32::offset(layer), Poly32::floats(layer), d_out, stream);
}

extern "C" int affnet_probe_hardnet_f43_layer(affnet_ctx* ctx, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patch || !d_out || layer < 0 || layer > 5) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_f43_layer: layer 0 .. 5");
    return aff_hardnet_poly_patches(ctx, d_packed, d_patch, 1, d_out, nullptr, layer, (hipStream_t)stream, AFFNET_DESC_FORM_F43);
}

extern "C" int affnet_probe_hardnet_f43_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patches || !d_out || !d_scratch || n < 1 || n > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_f43_forward: bad argument");
    return aff_hardnet_poly_patches(ctx, d_packed, d_patches, n, d_out, d_scratch, -1, (hipStream_t)stream, AFFNET_DESC_FORM_F43);
}

extern "C" int affnet_probe_hardnet_f43_u(affnet_ctx* ctx, const float* d_packed, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_out || (layer != 1 && layer != 3)) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_f43_u: layer 1 or 3");
    return probe_derived_u(ctx, AFFNET_NET_HARDNET, TRUNK_WINO_F43, d_packed, F43::BASE + F43::offset(layer), F43::floats(layer), d_out, stream);
}

// Descriptor form 3 (AFFNET_DESC_FORM_F43_CONV5): the trunk's layers 0 .. 4, the whole forward, conv5's kernel alone on caller-made slots, and its derived weights
extern "C" int affnet_probe_hardnet_c5_trunk_layer(affnet_ctx* ctx, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patch || !d_out || layer < 0 || layer > 4) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_c5_trunk_layer: layer 0 .. 4");
    return aff_hardnet_poly_patches(ctx, d_packed, d_patch, 1, d_out, nullptr, layer, (hipStream_t)stream, AFFNET_DESC_FORM_F43_CONV5);
}

extern "C" int affnet_probe_hardnet_c5_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patches || !d_out || !d_scratch || n < 1 || n > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_c5_forward: bad argument");
    return aff_hardnet_poly_patches(ctx, d_packed, d_patches, n, d_out, d_scratch, -1, (hipStream_t)stream, AFFNET_DESC_FORM_F43_CONV5);
}

extern "C" int affnet_probe_hardnet_c5_layer(affnet_ctx* ctx, const float* d_packed, float* d_slots, int n, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_slots || n < 1 || n > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_c5_layer: bad argument");
    if (ctx->arith != AFFNET_ARITH_FP32_MFMA) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_c5_layer: AFFNET_ARITH_FP32_MFMA only");
    const NetLayout L = net_layout(AFFNET_NET_HARDNET);
    const float* u;
    const int rc = aff_derive_u(ctx, AFFNET_NET_HARDNET, TRUNK_WINO_F43_C5, d_packed, L, (hipStream_t)stream, &u);
    if (rc) return rc;
    Conv5Args v;
    v.io = d_slots; v.U = u + F43C5::BASE; v.bias = d_packed + L.b_off[5];
    v.count = nullptr; v.n_max = n; v.row_begin = 0; v.row_end = n;
    v.skip_cnt = nullptr; v.skip_n = 0; v.dbg_time = nullptr;
    return aff_hardnet_conv5_f43(ctx, v, aff_cdiv(n, 4), 1, false, (hipStream_t)stream);
}

extern "C" int affnet_probe_hardnet_c5_u(affnet_ctx* ctx, const float* d_packed, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_out) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_c5_u: null argument");
    return probe_derived_u(ctx, AFFNET_NET_HARDNET, TRUNK_WINO_F43_C5, d_packed, F43C5::BASE, F43C5::FLOATS, d_out, stream);
}

// Descriptor form 4 (AFFNET_DESC_FORM_F43_CONV1): the trunk's layers 1 .. 4 and the whole forward
extern "C" int affnet_probe_hardnet_c1_trunk_layer(affnet_ctx* ctx, const float* d_packed, const float* d_patch, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patch || !d_out || layer < 1 || layer > 4) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_c1_trunk_layer: layer 1 .. 4");
    return aff_hardnet_poly_patches(ctx, d_packed, d_patch, 1, d_out, nullptr, layer, (hipStream_t)stream, AFFNET_DESC_FORM_F43_CONV1);
}

extern "C" int affnet_probe_hardnet_c1_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, int n, float* d_out, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_patches || !d_out || !d_scratch || n < 1 || n > 65535) return aff_fail(ctx, AFFNET_ERR_INVALID, "probe_hardnet_c1_forward: bad argument");
    return aff_hardnet_poly_patches(ctx, d_packed, d_patches, n, d_out, d_scratch, -1, (hipStream_t)stream, AFFNET_DESC_FORM_F43_CONV1);
}
