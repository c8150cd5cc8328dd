// The packed weight blob (include/affnet_hip.h: affnet_cnn32_packed_floats): its sections and offsets, the element order of every
// section, and the Winograd weight transform.  The one contract between the host packer (weights_pack.hip) and the kernels
// (cnn32.hip, cnn_trunk.h, cnn_heads.hip, cnn_mfma.h, fullconv.hip).  Plain arithmetic, no HIP header: compiles as C++ on the host as well.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/affnet_hip.h"

#ifdef __HIPCC__
#define AFF_HOST_DEVICE __host__ __device__
#else
#define AFF_HOST_DEVICE
#endif

#define HEAD_K 8192             // contraction length of HardNet's head: k = pixel * 128 + channel (the trunk kernel's output order)
#define H2_TAIL 4               // floats behind a two-term copy: [0] = 2^-e, the power of two that undoes the copy's scale (exact)
#define S3_LAYER_MASK 0x3E      // which layers have a split copy / run on split operands (bit i = conv i): conv1 .. conv5 of HardNet

// ---- element orders -----------------------------------------------------------------------------------
// fp32 weights [p][cin/16][kq = (c/4)%4][cout][c%4]: input channels interleaved by 4 like the LDS activations, so that one 16-byte load
// of lane (cout, kq) is the weight operand of four MFMA k-steps.  p = one of the 9 taps (ky * 3 + kx), or one of the 16 Winograd
// transform positions xi = 4 i + j of U = G g G^T; FullConv's dense 8 x 8 head uses it with p = ky and rows n = o * 8 + kx.
constexpr size_t w_tap_index(int p, int c, int n, int cin, int cout) {
    return ((((size_t)p * (cin / 16) + c / 16) * 4 + (c / 4) % 4) * cout + n) * 4 + c % 4;
}

// Split weights [step][term][kq][cout][8] in 16-bit elements (three bf16 terms or two fp16 terms): lane (cout, kq) of the k = 32 matrix
// instruction's weight operand = 8 consecutive input channels of one term.  A step is (tap, group of 32 input channels); with 16 input
// channels two taps share a step (kq = 2 * (tap % 2) + c / 8: 9 taps in 5 steps, the last half step stays zero).
constexpr size_t w_split_index(int tap, int c, int term, int n, int cin, int cout, int terms) {
    const int step = cin == 16 ? tap / 2 : tap * (cin / 32) + c / 32;
    const int kq = cin == 16 ? (tap % 2) * 2 + c / 8 : (c % 32) / 8;
    return ((((size_t)step * terms + term) * 4 + kq) * cout + n) * 8 + c % 8;
}

// floats occupied by the split copy of a cin x cout 3x3 layer (8 16-bit elements = 4 floats)
constexpr size_t s3_floats(int cin, int cout, int terms = 3) { return (size_t)(cin == 16 ? 5 : 9 * (cin / 32)) * terms * 4 * cout * 4; }

// HardNet's head GEMM (8192 x 128), fp32 [k/16][(k/4)%4][n][k%4] and split [k/32][term][kq = (k%32)/8][n][k%8]: the orders above with one tap
constexpr size_t head_index(size_t k, int n) { return w_tap_index(0, (int)k, n, HEAD_K, 128); }
constexpr size_t head_split_index(size_t k, int term, int n, int terms) { return w_split_index(0, (int)k, term, n, HEAD_K, 128, terms); }

// ---- sections -----------------------------------------------------------------------------------------
struct NetLayout {
    int cb;                 // base width: 16 (AffNet/OriNet) or 32 (HardNet)
    int cin[6], cout[6];
    size_t w_off[6], b_off[6];   // conv0 [tap (12, rows 9..11 zero)][cout]; conv1 .. conv5 w_tap_index over 9 taps; bias [cout]
    size_t head_w, head_b;  // head weights / bias (HardNet: BN-folded, head_index + bias[128]; AffNet / OriNet [o][pixel][channel]; FullConv w_tap_index, 32 rows)
    size_t w_s3[6];         // AFFNET_ARITH_FP32_SPLIT3 (0 = none): conv weights once more as three bf16 terms, w_split_index
    size_t head_s3;         // HardNet only: the BN-folded head weights as three bf16 terms, head_split_index
    size_t w_h2[6];         // AFFNET_ARITH_FP32_SPLIT2H (0 = none): the same layers as TWO fp16 terms of 2^e * w (e per layer: the largest |w| of the layer lands in
                            // [2^13, 2^14)), followed by H2_TAIL floats whose first is 2^-e (the loop's output scale)
    size_t head_h2;         // HardNet only: the head weights as two fp16 terms + H2_TAIL floats (2^-e first)
    size_t w_wino[6];       // HardNet conv1 / conv3 / conv5 (0 = none): the Winograd-transformed fp32 weights U = G g G^T, w_tap_index over 16
                            // transform positions.  LAST in the blob: every older offset keeps its value
    size_t total;
};

static inline NetLayout net_layout(int kind) {
    NetLayout L;
    L.cb = (kind == AFFNET_NET_HARDNET) ? 32 : 16;
    const int ch[7] = {1, L.cb, L.cb, 2 * L.cb, 2 * L.cb, 4 * L.cb, 4 * L.cb};
    size_t off = 0;
    for (int i = 0; i < 6; ++i) {
        L.cin[i] = ch[i]; L.cout[i] = ch[i + 1];
        L.w_off[i] = off; off += (i == 0) ? (size_t)12 * ch[1] : (size_t)9 * ch[i] * ch[i + 1];   // conv0: K = 9 padded to 12
        L.b_off[i] = off; off += ch[i + 1];
        off = (off + 3) & ~(size_t)3;
    }
    L.head_w = off;
    if (kind == AFFNET_NET_AFFNET) { off += 3 * 4096; L.head_b = off; off += 4; }
    else if (kind == AFFNET_NET_AFFNET_FULLCONV) { off += 8 * 64 * 32; L.head_b = off; off += 4; }
    else if (kind == AFFNET_NET_ORINET) { off += 2 * 4096; L.head_b = off; off += 4; }
    else { off += (size_t)HEAD_K * 128; L.head_b = off; off += 128; }
    for (int i = 0; i < 6; ++i) {
        L.w_s3[i] = 0;
        const bool has = (kind == AFFNET_NET_HARDNET && ((S3_LAYER_MASK >> i) & 1)) ||
                         ((kind == AFFNET_NET_AFFNET || kind == AFFNET_NET_ORINET || kind == AFFNET_NET_AFFNET_FULLCONV) && i >= 1);     // 16-channel trunks: conv1 .. conv5
        if (has) { L.w_s3[i] = off; off += s3_floats(L.cin[i], L.cout[i]); }
    }
    L.head_s3 = 0;
    if (kind == AFFNET_NET_HARDNET) { L.head_s3 = off; off += (size_t)HEAD_K * 128 * 3 / 2; }
    for (int i = 0; i < 6; ++i) {
        L.w_h2[i] = 0;
        if (L.w_s3[i]) { L.w_h2[i] = off; off += s3_floats(L.cin[i], L.cout[i], 2) + H2_TAIL; }
    }
    L.head_h2 = 0;
    if (kind == AFFNET_NET_HARDNET) { L.head_h2 = off; off += (size_t)HEAD_K * 128 + H2_TAIL; }
    for (int i = 0; i < 6; ++i) {
        L.w_wino[i] = 0;
        if (kind == AFFNET_NET_HARDNET && (i == 1 || i == 3 || i == 5)) { L.w_wino[i] = off; off += (size_t)16 * L.cin[i] * L.cout[i]; }
    }
    L.total = off;
    return L;
}

struct NetOffsets {        // device-side copy of the offsets (by-value kernel argument)
    int w[6], b[6], head_w, head_b;
    int w_s3[6];           // the split copy of the ACTIVE arithmetic mode (three bf16 terms or two fp16 terms)
    int head_s3;
    int w_wino[3];         // Winograd-transformed weights of conv1 / conv3 / conv5 (HardNet; 0 = none)
};

static inline NetOffsets to_offsets(const NetLayout& L, int arith = AFFNET_ARITH_FP32_SPLIT3) {
    NetOffsets o;
    const bool h2 = arith == AFFNET_ARITH_FP32_SPLIT2H;
    for (int i = 0; i < 6; ++i) { o.w[i] = (int)L.w_off[i]; o.b[i] = (int)L.b_off[i]; }
    o.head_w = (int)L.head_w; o.head_b = (int)L.head_b;
    for (int i = 0; i < 6; ++i) o.w_s3[i] = (int)(h2 ? L.w_h2[i] : L.w_s3[i]);
    o.head_s3 = (int)(h2 ? L.head_h2 : L.head_s3);
    for (int i = 0; i < 3; ++i) o.w_wino[i] = (int)L.w_wino[2 * i + 1];
    return o;
}

// ---- HardTFeat (tfeat.hip): a blob of its own (affnet_tfeat_packed_floats), no BatchNorm to fold ---------------------------------------
//   conv1 1 -> 32, 7 x 7     [k = ky * 7 + kx (52, rows 49..51 zero)][n]: the B operand of 13 MFMA k-steps;   bias [32]
//   conv2 32 -> 64, 6 x 6    w_tap_index over 36 taps p = ky * 6 + kx, cin 32, cout 64;                          bias [64]
//   classifier 64 -> 128, 8 x 8 as a (4096 x 128) GEMM: k = (y * 8 + x) * 64 + c, the order in which the trunk kernel stores conv2's output
//                            (the reference flattens as c * 64 + y * 8 + x: the packer transposes, callers never see k), in the head
//                            order [k/16][(k/4)%4][n][k%4];                                                        bias [128]
#define TFEAT_K1 52             // conv1's K = 49 taps padded to a multiple of the MFMA's 4
#define TFEAT_HEAD_K 4096       // contraction length of the classifier
constexpr size_t tfeat_c1_index(int k, int n) { return (size_t)k * 32 + n; }
constexpr size_t tfeat_c2_index(int p, int c, int n) { return w_tap_index(p, c, n, 32, 64); }
constexpr size_t tfeat_head_index(int pixel, int c, int n) { return w_tap_index(0, pixel * 64 + c, n, TFEAT_HEAD_K, 128); }

struct TfeatLayout {
    size_t c1_w, c1_b, c2_w, c2_b, head_w, head_b, total;
};

static inline TfeatLayout tfeat_layout() {
    TfeatLayout L;
    size_t off = 0;
    L.c1_w = off; off += (size_t)TFEAT_K1 * 32;
    L.c1_b = off; off += 32;
    L.c2_w = off; off += (size_t)36 * 32 * 64;
    L.c2_b = off; off += 64;
    L.head_w = off; off += (size_t)TFEAT_HEAD_K * 128;
    L.head_b = off; off += 128;
    L.total = off;
    return L;
}

// ---- Winograd F(2x2, 3x3) weight transform --------------------------------------------------------------
// U = G g G^T of one 3x3 filter g[ky * 3 + kx] into U[xi = 4 i + j], along x and then along y, one fp32 rounding per operation (the
// library is built with -ffp-contract=off).  The single definition of the operation order: the packer (HardNet's Winograd section) and
// wino_derive_u_kernel (OriNet) call it, tools/winograd_numerics.py: weight_transform mirrors it and the tests compare the two bit for bit.
AFF_HOST_DEVICE inline void wino_g_axis(float g0, float g1, float g2, float* o, int stride) {
    const float s = g0 + g2;
    o[0] = g0; o[stride] = 0.5f * (s + g1); o[2 * stride] = 0.5f * (s - g1); o[3 * stride] = g2;
}
AFF_HOST_DEVICE inline void wino_weight_transform(const float g[9], float U[16]) {
    float t[12];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) wino_g_axis(g[3 * ky], g[3 * ky + 1], g[3 * ky + 2], t + 4 * ky, 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) wino_g_axis(t[j], t[4 + j], t[8 + j], U + j, 4);
}

// ---- polyphase Winograd F(2x2, 2x2) weight transform of a 3x3 stride-2 layer (HardNet form 1: conv2 / conv4) --------------------------
// Along an axis taps 0 and 2 meet the odd input samples and form a 2-tap stride-1 filter, run as F(2, 2) with the weights (g0, g0 + g2, g2); tap 1 meets
// the even samples and serves both outputs of a tile as it is: (g0, g0 + g2, g2 | g1, g1), no constant but 1.  U[xi] of one filter g[ky * 3 + kx], along x
// and then along y, one fp32 rounding per sum; positions xi = 3 i + j (odd rows, odd columns: 9), 9 + 2 i + j (odd rows, even columns: 6),
// 15 + 3 i + j (even rows, odd columns: 6), 21 + 2 i + j (even / even: 4).  Stored in w_tap_index order over the 25 positions.  The single definition of
// the operation order: poly_derive_u_kernel (cnn_trunk_hardnet_poly.hip) calls it, tools/winograd_numerics.py: poly_weight_transform mirrors it.
#define POLY_XI 25
AFF_HOST_DEVICE inline void poly_weight_transform(const float g[9], float U[POLY_XI]) {
    float t[3][3];                              // along x, odd phase: t[ky][j]; the even phase is g[3 ky + 1] itself
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) { t[ky][0] = g[3 * ky]; t[ky][1] = g[3 * ky] + g[3 * ky + 2]; t[ky][2] = g[3 * ky + 2]; }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float s = t[0][j] + t[2][j];
        U[j] = t[0][j]; U[3 + j] = s; U[6 + j] = t[2][j];                        // odd rows, odd columns
        U[15 + j] = t[1][j]; U[18 + j] = t[1][j];                                // even rows, odd columns
    }
    const float se = g[1] + g[7];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        U[9 + j] = g[1]; U[11 + j] = se; U[13 + j] = g[7];                       // odd rows, even columns
        U[21 + j] = g[4]; U[23 + j] = g[4];                                      // even rows, even columns
    }
}

// U of HardNet's conv2 (32 -> 64) and conv4 (64 -> 128), one after the other in the buffer the context owns (205 KB + 819 KB)
struct Poly32 {
    static constexpr int U2 = POLY_XI * 32 * 64, U4 = POLY_XI * 64 * 128, FLOATS = U2 + U4;
    static constexpr int PAIRS = 32 * 64 + 64 * 128;                             // (cin, cout) pairs of the two layers
    static constexpr int offset(int layer) { return layer == 2 ? 0 : U2; }
    static constexpr int floats(int layer) { return layer == 2 ? U2 : U4; }
};

// ---- Winograd F(4x4, 3x3) weight transform (HardNet form 2: conv3; conv1 is derived as well) ---------------------------------------------
// Standard F(4, 3) on the points 0, +-1, +-2.  Along an axis U = G g with G's rows (1/4, 0, 0), (-1/6)(1, 1, 1), (-1/6)(1, -1, 1), (1/24, 1/12, 1/6),
// (1/24, -1/12, 1/6), (0, 0, 1), in ONE operation order, one fp32 rounding per operation (1/6, 1/12, 1/24 are the nearest floats):
//   s = g0 + g2;  p = (1/24) g0 + (1/6) g2;  q = (1/12) g1:   (0.25 g0, (-1/6)(s + g1), (-1/6)(s - g1), p + q, p - q, g2)
// U[xi = 6 i + j] of one filter g[ky * 3 + kx], along x and then along y.  Stored in w_tap_index order over the 36 positions.  The single definition of the
// operation order: f43_derive_u_kernel (cnn_trunk_hardnet_f43.hip) calls it, tools/winograd_numerics.py: f43_weight_transform mirrors it.
#define F43_XI 36
AFF_HOST_DEVICE inline void f43_g_axis(float g0, float g1, float g2, float* o, int stride) {
    const float c6 = 1.0f / 6.0f, c12 = 1.0f / 12.0f, c24 = 1.0f / 24.0f;
    const float s = g0 + g2;
    const float p = c24 * g0 + c6 * g2, q = c12 * g1;
    o[0] = 0.25f * g0; o[stride] = -c6 * (s + g1); o[2 * stride] = -c6 * (s - g1);
    o[3 * stride] = p + q; o[4 * stride] = p - q; o[5 * stride] = g2;
}
AFF_HOST_DEVICE inline void f43_weight_transform(const float g[9], float U[F43_XI]) {
    float t[18];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) f43_g_axis(g[3 * ky], g[3 * ky + 1], g[3 * ky + 2], t + 6 * ky, 1);
#pragma unroll
    for (int j = 0; j < 6; ++j) f43_g_axis(t[j], t[6 + j], t[12 + j], U + j, 6);
}

// U of HardNet's conv1 (32 -> 32) and conv3 (64 -> 64) in F(4x4, 3x3), one after the other BEHIND Poly32's floats in the same context-owned buffer (144 KB + 576 KB):
// the form 2 trunk takes one derived-weights pointer (CnnArgs::wino_u) and finds both families behind it
struct F43 {
    static constexpr int U1 = F43_XI * 32 * 32, U3 = F43_XI * 64 * 64, FLOATS = U1 + U3;
    static constexpr int PAIRS = 32 * 32 + 64 * 64;                              // (cin, cout) pairs of the two layers
    static constexpr int BASE = Poly32::FLOATS;                                  // float offset of the family in the context's buffer
    static constexpr int offset(int layer) { return layer == 1 ? 0 : U1; }       // ... of a layer inside the family
    static constexpr int floats(int layer) { return layer == 1 ? U1 : U3; }
};
