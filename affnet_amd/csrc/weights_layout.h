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
// derive_u_pair (below) call it, tools/winograd_numerics.py: weight_transform mirrors it and the tests compare the two bit for bit.
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
// the operation order: derive_u_pair (below) calls it, tools/winograd_numerics.py: poly_weight_transform mirrors it.
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

// ---- Winograd F(4x4, 3x3) weight transform (HardNet form 2: conv3; conv1 is derived as well) ---------------------------------------------
// Standard F(4, 3) on the points 0, +-1, +-2.  Along an axis U = G g with G's rows (1/4, 0, 0), (-1/6)(1, 1, 1), (-1/6)(1, -1, 1), (1/24, 1/12, 1/6),
// (1/24, -1/12, 1/6), (0, 0, 1), in ONE operation order, one fp32 rounding per operation (1/6, 1/12, 1/24 are the nearest floats):
//   s = g0 + g2;  p = (1/24) g0 + (1/6) g2;  q = (1/12) g1:   (0.25 g0, (-1/6)(s + g1), (-1/6)(s - g1), p + q, p - q, g2)
// U[xi = 6 i + j] of one filter g[ky * 3 + kx], along x and then along y.  Stored in w_tap_index order over the 36 positions.  The single definition of the
// operation order: derive_u_pair (below) calls it, tools/winograd_numerics.py: f43_weight_transform mirrors it.
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

// ---- derived weights: sections, tables, the derivation routine --------------------------------------------------------------------------
// Transformed weights that are NOT blob sections (the blobs' sizes and hashes are pinned, and a blob packed by an older library stays valid): derived on the device from
// the blob's BN-folded fp32 taps into the one buffer a context owns (DerivedU below), in front of every trunk launch that reads them (derive_u.hip).  A section = U of one
// layer in one family, that family's positions in w_tap_index order.  Everything about a section is in its table row; Wino16 / Poly32 / F43 are views of the tables.
enum { DERIVED_WINO = 0, DERIVED_POLY = 1, DERIVED_F43 = 2 };   // Winograd F(2x2, 3x3): 16 positions; polyphase F(2x2, 2x2): POLY_XI; Winograd F(4x4, 3x3): F43_XI
constexpr int derived_xi(int family) { return family == DERIVED_WINO ? 16 : (family == DERIVED_POLY ? POLY_XI : F43_XI); }
struct DerivedSection {
    int layer, cin, cout;       // source: conv `layer` of the blob (9 taps in w_tap_index order at NetOffsets::w[layer]), cin -> cout
    int family;                 // DERIVED_*
    int pair0;                  // first pair of the section = first thread of a launch; pair0 + w_tap_index(0, c, n, cin, cout) is pair (c, n): the fragment order, contiguous per wave
    int dst;                    // float offset of the section from the table's base
};
constexpr int derived_floats(const DerivedSection& s) { return derived_xi(s.family) * s.cin * s.cout; }
#define DERIVED_MAX 5
struct DerivedTable {           // by-value kernel argument
    int n, pairs, floats;       // sections; pairs (= threads) of all sections; floats from the base to the end of the last section
    DerivedSection s[DERIVED_MAX];
};
// `t` with one more section behind its last: conv `layer` of a trunk of base width cb (NetLayout's channel counts) in `family`
constexpr DerivedTable derived_add(DerivedTable t, int cb, int layer, int family) {
    const DerivedSection s = {layer, cb << ((layer - 1) / 2), cb << (layer / 2), family, t.pairs, t.floats};
    t.s[t.n++] = s; t.pairs += s.cin * s.cout; t.floats += derived_floats(s);
    return t;
}
// A 16-channel net (AffNet, OriNet): conv1 / conv3 / conv5 in Winograd F(2x2, 3x3), behind them (appended later) the stride-2 layers conv2 / conv4 as polyphase Winograd.  600 KB.
constexpr DerivedTable derived_trunk16() {
    return derived_add(derived_add(derived_add(derived_add(derived_add(DerivedTable{}, 16, 1, DERIVED_WINO), 16, 3, DERIVED_WINO), 16, 5, DERIVED_WINO), 16, 2, DERIVED_POLY), 16, 4, DERIVED_POLY);
}
// HardNet descriptor form 1: conv2 / conv4 as polyphase Winograd (205 KB + 819 KB)
constexpr DerivedTable derived_hardnet_poly() { return derived_add(derived_add(DerivedTable{}, 32, 2, DERIVED_POLY), 32, 4, DERIVED_POLY); }
// HardNet's conv1 / conv3 in Winograd F(4x4, 3x3) (144 KB + 576 KB; conv1's is read by descriptor form 4 only) ...
constexpr DerivedTable derived_hardnet_f43() { return derived_add(derived_add(DerivedTable{}, 32, 1, DERIVED_F43), 32, 3, DERIVED_F43); }
// ... and what descriptor form 2 reads: those directly BEHIND form 1's polyphase sections - its trunk takes one derived-weights pointer (CnnArgs::wino_u) and finds both there
constexpr DerivedTable derived_hardnet_form2() { return derived_add(derived_add(derived_hardnet_poly(), 32, 1, DERIVED_F43), 32, 3, DERIVED_F43); }
// ... and descriptor form 3: form 2's table with conv5 (128 -> 128) in F(4x4, 3x3) behind it (2.36 MB), which hardnet_conv5_f43_kernel reads; its trunk reads form 2's sections where form 2's does
constexpr DerivedTable derived_hardnet_form3() { return derived_add(derived_hardnet_form2(), 32, 5, DERIVED_F43); }
// the section of conv `layer` (layer -1: not in the table)
constexpr DerivedSection derived_layer(const DerivedTable& t, int layer) {
    for (int i = 0; i < t.n; ++i)
        if (t.s[i].layer == layer) return t.s[i];
    return DerivedSection{-1, 0, 0, 0, 0, 0};
}
// the section that pair e < t.pairs belongs to
constexpr DerivedSection derived_section(const DerivedTable& t, int e) {
    DerivedSection s = t.s[0];
    for (int i = 1; i < DERIVED_MAX; ++i)
        if (i < t.n && e >= t.s[i].pair0) s = t.s[i];
    return s;
}
// Every section begins and ends on a multiple of 256 pairs: the 256 threads of a workgroup of the derivation kernel work on ONE section (one family: no divergence)
constexpr bool derived_by_workgroups(const DerivedTable& t, int i = 0) {
    return i == t.n || (t.s[i].pair0 % 256 == 0 && t.s[i].cin * t.s[i].cout % 256 == 0 && derived_by_workgroups(t, i + 1));
}
static_assert(derived_by_workgroups(derived_trunk16()) && derived_by_workgroups(derived_hardnet_poly()) && derived_by_workgroups(derived_hardnet_f43()) &&
              derived_by_workgroups(derived_hardnet_form2()) && derived_by_workgroups(derived_hardnet_form3()), "a 256-thread workgroup of derive_u_kernel stays within one section");

// What the trunk kernels address the sections of a table through
template <DerivedTable (*T)()>
struct DerivedView {
    static constexpr int FLOATS = T().floats, PAIRS = T().pairs;
    static constexpr int offset(int layer) { return derived_layer(T(), layer).dst; }
    static constexpr int floats(int layer) { return derived_floats(derived_layer(T(), layer)); }
};
struct Wino16 : DerivedView<derived_trunk16> { static constexpr int NB1 = 2, NB3 = 1; };   // (tile block, channel block) passes per wave of conv1 / conv3: 16 x 1 / 8, 4 x 2 / 8
typedef DerivedView<derived_hardnet_poly> Poly32;
struct F43 : DerivedView<derived_hardnet_f43> { static constexpr int BASE = Poly32::FLOATS; };   // float offset of the family from form 2's derived-weights pointer; offset(layer) is inside the family
static_assert(derived_hardnet_form2().s[2].dst == F43::BASE + F43::offset(1) && derived_hardnet_form2().s[3].dst == F43::BASE + F43::offset(3) &&
              derived_hardnet_form2().floats == F43::BASE + F43::FLOATS, "form 2's table = Poly32 with F43 at F43::BASE");
struct F43C5 {                                                                                   // conv5 of descriptor form 3: float offset from form 3's derived-weights pointer, and its size
    static constexpr int BASE = derived_hardnet_form2().floats, FLOATS = F43_XI * 128 * 128;
};
static_assert(derived_hardnet_form3().n == 5 && derived_hardnet_form3().s[4].dst == F43C5::BASE && derived_hardnet_form3().floats == F43C5::BASE + F43C5::FLOATS, "form 3's table = form 2's with conv5 at F43C5::BASE");

// The context's buffer of derived weights, in floats: a region per net, each the base of that net's table(s)
struct DerivedU {
    static constexpr int AFFNET = 0, ORINET = AFFNET + Wino16::FLOATS;               // derived_trunk16() each
    static constexpr int HARDNET = ORINET + Wino16::FLOATS;                          // derived_hardnet_poly() / derived_hardnet_form2()
    static constexpr int HARDNET_F43 = HARDNET + F43::BASE;                          // ... whose F(4x4, 3x3) part is derived_hardnet_f43()
    static constexpr int HARDNET_C5 = HARDNET + F43C5::BASE;                         // ... and behind it conv5 of descriptor form 3 (derived_hardnet_form3())
    static constexpr int FLOATS = HARDNET_C5 + F43C5::FLOATS;                        // 5.4 MB
    static constexpr int region(int kind) { return kind == AFFNET_NET_AFFNET ? AFFNET : (kind == AFFNET_NET_ORINET ? ORINET : HARDNET); }
};
static_assert(DerivedU::AFFNET == 0 && DerivedU::ORINET - DerivedU::AFFNET == derived_trunk16().floats && DerivedU::HARDNET - DerivedU::ORINET == derived_trunk16().floats &&
              DerivedU::FLOATS - DerivedU::HARDNET == derived_hardnet_form3().floats && DerivedU::FLOATS == 2 * Wino16::FLOATS + Poly32::FLOATS + F43::FLOATS + F43C5::FLOATS,
              "the regions are disjoint, in this order, and fill the buffer");
static_assert(DerivedU::ORINET % 64 == 0 && DerivedU::HARDNET % 64 == 0 && DerivedU::HARDNET_F43 % 64 == 0 && DerivedU::HARDNET_C5 % 64 == 0, "every region starts on a 256-byte boundary, as an allocation of its own would");
// The work of thread e of a derivation launch over table t: pair e - pair0 of its section is pair (c, n) with e - pair0 == w_tap_index(0, c, n, cin, cout), and a position
// (tap or transform position) p of that pair lies p planes of cin * cout floats further: w_tap_index(p, c, n, cin, cout) == p * cin * cout + w_tap_index(0, c, n, cin, cout).
// So: the pair's 9 taps of the blob (w_off = NetOffsets::w) through the family's transform into that family's positions at U + dst, plane by plane.  The section is looked
// up for the first pair of e's group of 256 (derived_by_workgroups): on the device that is the workgroup's, a scalar.
static_assert(w_tap_index(7, 21, 13, 32, 64) == 7 * 32 * 64 + w_tap_index(0, 21, 13, 32, 64) && w_tap_index(35, 63, 63, 64, 64) == 35 * 64 * 64 + w_tap_index(0, 63, 63, 64, 64),
              "a position is a plane of cin * cout floats");
AFF_HOST_DEVICE inline void derive_u_pair(const DerivedTable& t, int e, const float* packed, const int (&w_off)[6], float* U) {
    if (e >= t.pairs) return;
    const DerivedSection s = derived_section(t, e & ~255);
    const int plane = s.cin * s.cout;
    const float* src = packed + w_off[s.layer] + (e - s.pair0);
    float* dst = U + s.dst + (e - s.pair0);
    float g[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) g[tap] = src[(size_t)tap * plane];
    float u[F43_XI];                                    // the largest family
    if (s.family == DERIVED_WINO) wino_weight_transform(g, u);
    else if (s.family == DERIVED_POLY) poly_weight_transform(g, u);
    else f43_weight_transform(g, u);
#pragma unroll
    for (int xi = 0; xi < F43_XI; ++xi)
        if (xi < derived_xi(s.family)) dst[(size_t)xi * plane] = u[xi];
}
