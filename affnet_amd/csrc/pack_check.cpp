// Stand-alone host check of the weight packer (weights_pack.hip compiled as C++) under the address and undefined-behaviour sanitizers:
// build_pack_check.sh builds and runs it.  No GPU, no HIP runtime.  Every array has exactly the size the boundary documents (new
// float[exact]), so an over-read or over-write by a single element is reported.
#include <math.h>
#include <stdio.h>

#include <initializer_list>
#include <memory>

#include "../../include/affnet_hip.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "pack_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct State {                      // one network's state dict, shapes as in include/affnet_hip.h
    std::unique_ptr<float[]> conv[6], mean[6], var[6], head_w, head_b, hbm, hbv, out;
    const float *conv_p[6], *mean_p[6], *var_p[6];
    size_t conv_n[6], total;
};

static uint32_t lcg = 12345u;
static float rnd() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) / (float)(1 << 24) - 0.5f; }
static std::unique_ptr<float[]> filled(size_t n, float scale, float offset) {
    std::unique_ptr<float[]> p(new float[n]);
    for (size_t i = 0; i < n; ++i) p[i] = rnd() * scale + offset;
    return p;
}

static void make_state(int kind, State& s) {
    const int cb = kind == AFFNET_NET_HARDNET ? 32 : 16, ch[7] = {1, cb, cb, 2 * cb, 2 * cb, 4 * cb, 4 * cb};
    for (int i = 0; i < 6; ++i) {
        s.conv_n[i] = (size_t)ch[i + 1] * ch[i] * 9;
        s.conv[i] = filled(s.conv_n[i], 0.2f, 0.f); s.mean[i] = filled(ch[i + 1], 1.f, 0.f); s.var[i] = filled(ch[i + 1], 1.f, 1.f);      // var in [0.5, 1.5)
        s.conv_p[i] = s.conv[i].get(); s.mean_p[i] = s.mean[i].get(); s.var_p[i] = s.var[i].get();
    }
    const int no = kind == AFFNET_NET_ORINET ? 2 : 3;
    if (kind == AFFNET_NET_HARDNET) { s.head_w = filled((size_t)128 * 128 * 64, 0.02f, 0.f); s.hbm = filled(128, 1.f, 0.f); s.hbv = filled(128, 1.f, 1.f); }
    else { s.head_w = filled((size_t)no * 64 * 64, 0.1f, 0.f); s.head_b = filled(no, 1.f, 0.f); }
    s.total = affnet_cnn32_packed_floats(kind);
    s.out.reset(new float[s.total]);
}

static int pack(int kind, State& s) {
    return affnet_cnn32_pack_weights(kind, s.conv_p, s.mean_p, s.var_p, s.head_w.get(), s.head_b.get(), s.hbm.get(), s.hbv.get(), s.out.get());
}

static int check_kind(int kind) {
    State s;
    make_state(kind, s);
    CHECK(s.total > 0 && pack(kind, s) == AFFNET_OK);
    size_t nonfinite = 0;
    for (size_t i = 0; i < s.total; ++i) nonfinite += !isfinite(s.out[i]);
    CHECK(nonfinite == 0);
    // the Winograd sections: HardNet conv1 / conv3 / conv5, appended in this order; nowhere else
    int64_t want = -1;
    for (int layer = -1; layer <= 6; ++layer) {
        const bool has = kind == AFFNET_NET_HARDNET && (layer == 1 || layer == 3 || layer == 5);
        const int64_t got = affnet_cnn32_winograd_offset(kind, layer);
        if (!has) { CHECK(got == -1); continue; }
        if (want < 0) want = (int64_t)s.total - 16 * (32 * 32 + 64 * 64 + 128 * 128);
        CHECK(got == want);
        want += 16 * (layer == 1 ? 32 * 32 : layer == 3 ? 64 * 64 : 128 * 128);
    }
    CHECK(affnet_cnn32_winograd_offset(-1, 1) == -1 && affnet_cnn32_winograd_offset(4, 1) == -1 && affnet_cnn32_packed_floats(-1) == 0 && affnet_cnn32_packed_floats(4) == 0);
    // arguments the packer rejects
    float* const o = s.out.get();
    const float *hw = s.head_w.get(), *hb = s.head_b.get(), *m = s.hbm.get(), *v = s.hbv.get();
    CHECK(affnet_cnn32_pack_weights(kind, nullptr, s.mean_p, s.var_p, hw, hb, m, v, o) == AFFNET_ERR_INVALID);
    CHECK(affnet_cnn32_pack_weights(kind, s.conv_p, nullptr, s.var_p, hw, hb, m, v, o) == AFFNET_ERR_INVALID);
    CHECK(affnet_cnn32_pack_weights(kind, s.conv_p, s.mean_p, nullptr, hw, hb, m, v, o) == AFFNET_ERR_INVALID);
    CHECK(affnet_cnn32_pack_weights(kind, s.conv_p, s.mean_p, s.var_p, nullptr, hb, m, v, o) == AFFNET_ERR_INVALID);
    CHECK(affnet_cnn32_pack_weights(kind, s.conv_p, s.mean_p, s.var_p, hw, hb, m, v, nullptr) == AFFNET_ERR_INVALID);
    CHECK(affnet_cnn32_pack_weights(-1, s.conv_p, s.mean_p, s.var_p, hw, hb, m, v, o) == AFFNET_ERR_INVALID);
    CHECK(affnet_cnn32_pack_weights(4, s.conv_p, s.mean_p, s.var_p, hw, hb, m, v, o) == AFFNET_ERR_INVALID);
    if (kind == AFFNET_NET_HARDNET) {
        CHECK(affnet_cnn32_pack_weights(kind, s.conv_p, s.mean_p, s.var_p, hw, hb, nullptr, v, o) == AFFNET_ERR_INVALID);
        CHECK(affnet_cnn32_pack_weights(kind, s.conv_p, s.mean_p, s.var_p, hw, hb, m, nullptr, o) == AFFNET_ERR_INVALID);
    } else {
        CHECK(affnet_cnn32_pack_weights(kind, s.conv_p, s.mean_p, s.var_p, hw, nullptr, m, v, o) == AFFNET_ERR_INVALID);
    }
    // edge weights: the call returns and the sanitizers stay silent
    int edges = 0;
    const float saved = s.conv[3][7], saved_var = s.var[2][1];
    for (const float x : {INFINITY, NAN}) { s.conv[3][7] = x; CHECK(pack(kind, s) == AFFNET_OK); ++edges; }
    s.conv[3][7] = saved;
    s.var[2][1] = 0.f; CHECK(pack(kind, s) == AFFNET_OK); ++edges;
    s.var[2][1] = saved_var;
    for (const float scale : {0.f, 1e-30f, 1e30f}) {        // wmax == 0 (e = 0) and the two ends of the exponent clamp
        for (int i = 0; i < 6; ++i)
            for (size_t j = 0; j < s.conv_n[i]; ++j) s.conv[i][j] = scale * ((j & 1) ? -1.f : 1.f);
        CHECK(pack(kind, s) == AFFNET_OK); ++edges;
    }
    printf("kind %d: %zu floats packed, %d edge cases and the rejected arguments as documented\n", kind, s.total, edges);
    return 0;
}

int main() {
    for (int kind = 0; kind <= AFFNET_NET_AFFNET_FULLCONV; ++kind)
        if (check_kind(kind)) return 1;
    return 0;
}
