// Host side of the packed weight blob: state dict -> BN-folded weights in the element orders of weights_layout.h.  Host arithmetic only
// (no kernel, no HIP call): built into the library with the other sources, and as plain C++ (-x c++) by build_pack_check.sh, which
// runs it under the address and undefined-behaviour sanitizers.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <memory>

#include "weights_layout.h"

extern "C" size_t affnet_cnn32_packed_floats(int net_kind) {
    if (net_kind < 0 || net_kind > AFFNET_NET_AFFNET_FULLCONV) return 0;
    return net_layout(net_kind).total;
}

extern "C" int64_t affnet_cnn32_winograd_offset(int net_kind, int layer) {
    if (net_kind < 0 || net_kind > AFFNET_NET_AFFNET_FULLCONV || layer < 0 || layer > 5) return -1;
    const NetLayout L = net_layout(net_kind);
    return L.w_wino[layer] ? (int64_t)L.w_wino[layer] : -1;
}

extern "C" size_t affnet_tfeat_packed_floats(void) { return tfeat_layout().total; }

// HardTFeat: no BatchNorm, so every weight is copied unchanged into the element orders of weights_layout.h (tfeat_c1_index, tfeat_c2_index,
// tfeat_head_index); conv1's rows 49..51 stay zero.
extern "C" int affnet_tfeat_pack_weights(const float* conv1_w, const float* conv1_b, const float* conv2_w, const float* conv2_b, const float* cls_w,
                                         const float* cls_b, float* h_out) {
    if (!conv1_w || !conv1_b || !conv2_w || !conv2_b || !cls_w || !cls_b || !h_out) return AFFNET_ERR_INVALID;
    const TfeatLayout L = tfeat_layout();
    memset(h_out, 0, L.total * sizeof(float));
    for (int n = 0; n < 32; ++n)                                // conv1 [n][1][7][7]
        for (int k = 0; k < 49; ++k) h_out[L.c1_w + tfeat_c1_index(k, n)] = conv1_w[n * 49 + k];
    memcpy(h_out + L.c1_b, conv1_b, 32 * sizeof(float));
    for (int n = 0; n < 64; ++n)                                // conv2 [n][c 32][6][6]
        for (int c = 0; c < 32; ++c)
            for (int p = 0; p < 36; ++p) h_out[L.c2_w + tfeat_c2_index(p, c, n)] = conv2_w[((size_t)n * 32 + c) * 36 + p];
    memcpy(h_out + L.c2_b, conv2_b, 64 * sizeof(float));
    for (int n = 0; n < 128; ++n)                               // classifier [n][c 64][8][8]
        for (int c = 0; c < 64; ++c)
            for (int p = 0; p < 64; ++p) h_out[L.head_w + tfeat_head_index(p, c, n)] = cls_w[((size_t)n * 64 + c) * 64 + p];
    memcpy(h_out + L.head_b, cls_b, 128 * sizeof(float));
    return AFFNET_OK;
}

namespace {

// BatchNorm2d(affine=False), eps 1e-5, eval mode, folded into `cout` filters of `k` weights: w * s (one multiply) and the bias -mean * s
void fold_bn(const float* w, const float* mean, const float* var, int cout, size_t k, float* folded, float* bias) {
    for (int n = 0; n < cout; ++n) {
        const float s = 1.0f / sqrtf(var[n] + 1e-5f);
        bias[n] = -mean[n] * s;
        for (size_t j = 0; j < k; ++j) folded[n * k + j] = w[n * k + j] * s;
    }
}

// f(n, c, t, weight) over BN-folded filters [cout][cin][taps], in memory order
template <typename F>
void for_each_weight(const float* w, int cout, int cin, int taps, F f) {
    for (int n = 0; n < cout; ++n)
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < taps; ++t) f(n, c, t, *w++);
}

// fp32 = three bf16 terms (round to nearest even, exact remainders) of the value the fp32 path uses; term `term` of weight (n, c, t) goes to dst[index(n, c, t, term)]
template <typename Index>
void pack_split3(const float* w, int cout, int cin, int taps, uint16_t* dst, Index index) {
    for_each_weight(w, cout, cin, taps, [&](int n, int c, int t, float r) {
        for (int term = 0; term < 3; ++term) {
            uint32_t u;
            memcpy(&u, &r, 4);
            const uint32_t hb = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
            float hf;
            memcpy(&hf, &hb, 4);
            r -= hf;                                                       // exact
            dst[index(n, c, t, term)] = (uint16_t)(hb >> 16);
        }
    });
}

// Two fp16 terms of 2^e * w: hi = fp16(2^e w), lo = fp16(2^e w - hi) (nearest even; the scaling is exact), e per filter bank such that the
// largest |w| lands in [2^13, 2^14) - both terms of every weight down to 2^-15 of the largest then sit in fp16's normal range.  e is clamped
// (2^-e must stay a normal fp32) and 0 for an all-zero or non-finite bank.  tail[0] = 2^-e, what the loop multiplies its sums with.
template <typename Index>
void pack_split2(const float* w, int cout, int cin, int taps, uint16_t* dst, float* tail, Index index) {
    float wmax = 0.0f;
    for (size_t j = 0; j < (size_t)cout * cin * taps; ++j) wmax = fmaxf(wmax, fabsf(w[j]));
    const int e = (wmax > 0.0f && std::isfinite(wmax)) ? std::min(100, std::max(-100, 13 - ilogbf(wmax))) : 0;
    tail[0] = ldexpf(1.0f, -e);
    auto f16_bits = [](float x) -> uint16_t { const _Float16 h = (_Float16)x; uint16_t u; memcpy(&u, &h, 2); return u; };
    for_each_weight(w, cout, cin, taps, [&](int n, int c, int t, float x) {
        x = ldexpf(x, e);
        const uint16_t hb = f16_bits(x);
        _Float16 hi;
        memcpy(&hi, &hb, 2);
        dst[index(n, c, t, 0)] = hb;
        dst[index(n, c, t, 1)] = f16_bits(x - (float)hi);
    });
}

}  // namespace

extern "C" int affnet_cnn32_pack_weights(int kind, const float* const* conv_w, const float* const* bn_mean, const float* const* bn_var,
                                         const float* head_w, const float* head_b, const float* head_bn_mean, const float* head_bn_var,
                                         float* out) {
    if (kind < 0 || kind > AFFNET_NET_AFFNET_FULLCONV || !conv_w || !bn_mean || !bn_var || !head_w || !out) return AFFNET_ERR_INVALID;
    if (kind == AFFNET_NET_HARDNET ? (!head_bn_mean || !head_bn_var) : !head_b) return AFFNET_ERR_INVALID;
    const NetLayout L = net_layout(kind);
    const size_t tmp_floats = kind == AFFNET_NET_HARDNET ? (size_t)HEAD_K * 128 : (size_t)9 * L.cin[5] * L.cout[5];      // the largest filter bank
    const std::unique_ptr<float[]> tmp(new (std::nothrow) float[tmp_floats]);
    if (!tmp) return AFFNET_ERR_INVALID;                       // (out of memory: the boundary has no code of its own for it)
    float* const w = tmp.get();                                 // the BN-folded filters of the layer in hand, [cout][cin][9] - every copy derives from it
    auto u16 = [&](size_t off) { return reinterpret_cast<uint16_t*>(out + off); };
    memset(out, 0, L.total * sizeof(float));
    for (int i = 0; i < 6; ++i) {
        const int ci = L.cin[i], co = L.cout[i];
        fold_bn(conv_w[i], bn_mean[i], bn_var[i], co, (size_t)ci * 9, w, out + L.b_off[i]);
        if (i == 0) for_each_weight(w, co, 1, 9, [&](int n, int, int t, float x) { out[L.w_off[0] + (size_t)t * co + n] = x; });      // [tap (12, rows 9..11 zero)][n]
        else for_each_weight(w, co, ci, 9, [&](int n, int c, int t, float x) { out[L.w_off[i] + w_tap_index(t, c, n, ci, co)] = x; });
        if (L.w_wino[i])                                        // U = G g G^T of the same folded taps, 16 transform positions in place of 9 taps
            for (int n = 0; n < co; ++n)
                for (int c = 0; c < ci; ++c) {
                    float U[16];
                    wino_weight_transform(w + ((size_t)n * ci + c) * 9, U);
                    for (int xi = 0; xi < 16; ++xi) out[L.w_wino[i] + w_tap_index(xi, c, n, ci, co)] = U[xi];
                }
        if (L.w_s3[i]) pack_split3(w, co, ci, 9, u16(L.w_s3[i]), [=](int n, int c, int t, int term) { return w_split_index(t, c, term, n, ci, co, 3); });
        if (L.w_h2[i])
            pack_split2(w, co, ci, 9, u16(L.w_h2[i]), out + L.w_h2[i] + s3_floats(ci, co, 2), [=](int n, int c, int t, int term) { return w_split_index(t, c, term, n, ci, co, 2); });
    }
    if (kind == AFFNET_NET_HARDNET) {
        // the head's filters [n 128][channel c 128][pixel t 64]: contraction index k = t * 128 + c, the trunk kernel's output order
        fold_bn(head_w, head_bn_mean, head_bn_var, 128, HEAD_K, w, out + L.head_b);
        for_each_weight(w, 128, 128, 64, [&](int n, int c, int t, float x) { out[L.head_w + head_index(t * 128 + c, n)] = x; });
        pack_split3(w, 128, 128, 64, u16(L.head_s3), [](int n, int c, int t, int term) { return head_split_index(t * 128 + c, term, n, 3); });
        pack_split2(w, 128, 128, 64, u16(L.head_h2), out + L.head_h2 + (size_t)HEAD_K * 128, [](int n, int c, int t, int term) { return head_split_index(t * 128 + c, term, n, 2); });
    } else if (kind == AFFNET_NET_AFFNET_FULLCONV) {
        // dense 8 x 8 head (architectures.py:652) as the A operand of fullconv_head_kernel's GEMM: rows n = o * 8 + kx (24 of 32
        // used, the rest stay zero), K = (ky, c)
        for (int o = 0; o < 3; ++o)
            for (int c = 0; c < 64; ++c)
                for (int ky = 0; ky < 8; ++ky)
                    for (int kx = 0; kx < 8; ++kx) out[L.head_w + w_tap_index(ky, c, o * 8 + kx, 64, 32)] = head_w[((size_t)o * 64 + c) * 64 + ky * 8 + kx];
        memcpy(out + L.head_b, head_b, 3 * sizeof(float));
    } else {
        const int no = kind == AFFNET_NET_AFFNET ? 3 : 2;
        // [o][pixel p][channel c]: (pixel, 4 consecutive channels) = what one lane of the conv5 epilogue owns (head_partials)
        for (int o = 0; o < no; ++o)
            for (int c = 0; c < 64; ++c)
                for (int pp = 0; pp < 64; ++pp) out[L.head_w + (size_t)o * 4096 + pp * 64 + c] = head_w[((size_t)o * 64 + c) * 64 + pp];
        memcpy(out + L.head_b, head_b, no * sizeof(float));
    }
    return AFFNET_OK;
}
