// Stand-alone host check of the weight packer (weights_pack.hip compiled as C++) and of the derived-weights tables and routine (weights_layout.h: derive_u_pair, the host
// side of derive_u_kernel) under the address and undefined-behaviour sanitizers: build_pack_check.sh builds and runs it.  No GPU, no HIP runtime.  Every array has exactly
// the size the boundary documents (new float[exact]), so an over-read or over-write by a single element is reported.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <memory>

#include "../../include/affnet_hip.h"
#include "weights_layout.h"

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

// ---- derived weights.  The layouts the trunk kernels read, as numbers: a table that moved a section fails here before it produces valid floats in the wrong place.
static_assert(Wino16::offset(1) == 0 && Wino16::offset(3) == 4096 && Wino16::offset(5) == 20480 && Wino16::offset(2) == 86016 && Wino16::offset(4) == 98816 && Wino16::FLOATS == 150016 && Wino16::PAIRS == 7936, "Wino16");
static_assert(Poly32::offset(2) == 0 && Poly32::offset(4) == 51200 && Poly32::FLOATS == 256000 && Poly32::PAIRS == 10240, "Poly32");
static_assert(F43::BASE == 256000 && F43::offset(1) == 0 && F43::offset(3) == 36864 && F43::FLOATS == 184320 && F43::PAIRS == 5120, "F43");
static_assert(F43C5::BASE == 440320 && F43C5::FLOATS == 589824 && derived_hardnet_form3().pairs == 15360 + 16384, "F43C5");

// Table t of a `kind` blob: derive_u_pair for every pair index into a destination of exactly want_floats floats; every float is written by the pair that owns it and by
// no other, and holds the family's transform of the 9 taps that plain (layer, tap, cin, cout) indexing finds in the blob.
static int check_derived(const char* name, int kind, const DerivedTable& t, int want_sections, size_t want_floats) {
    const NetLayout L = net_layout(kind); const NetOffsets off = to_offsets(L);
    CHECK(L.total == affnet_cnn32_packed_floats(kind) && t.n == want_sections && t.n <= DERIVED_MAX && (size_t)t.floats == want_floats && t.pairs % 256 == 0);
    const std::unique_ptr<float[]> blob = filled(L.total, 0.2f, 0.f), U(new float[want_floats]), want(new float[want_floats]);
    const std::unique_ptr<unsigned char[]> owned(new unsigned char[want_floats]());
    const float sentinel = -12345.f;                     // no transform of taps in [-0.1, 0.1) comes near it
    for (size_t i = 0; i < want_floats; ++i) U[i] = sentinel;
    size_t pairs = 0, floats = 0;
    for (int i = 0; i < t.n; ++i) {
        const DerivedSection& s = t.s[i];
        const int xi = s.family == DERIVED_WINO ? 16 : s.family == DERIVED_POLY ? 25 : 36;
        CHECK(s.layer >= 1 && s.layer <= 5 && s.cin == L.cin[s.layer] && s.cout == L.cout[s.layer] && (size_t)s.pair0 == pairs && s.family >= 0 && s.family <= DERIVED_F43);
        for (int c = 0; c < s.cin; ++c)
            for (int n = 0; n < s.cout; ++n, ++pairs) {
                float g[9], u[36];
                for (int tap = 0; tap < 9; ++tap) g[tap] = blob[L.w_off[s.layer] + w_tap_index(tap, c, n, s.cin, s.cout)];
                if (s.family == DERIVED_WINO) wino_weight_transform(g, u);
                else if (s.family == DERIVED_POLY) poly_weight_transform(g, u);
                else f43_weight_transform(g, u);
                const size_t e = s.pair0 + w_tap_index(0, c, n, s.cin, s.cout);        // distinct per pair, as the pair's floats are
                CHECK(e < (size_t)t.pairs);
                for (int p = 0; p < xi; ++p, ++floats) {  // the floats of this pair: nobody's yet, untouched so far
                    const size_t d = s.dst + w_tap_index(p, c, n, s.cin, s.cout);
                    CHECK(d < want_floats && !owned[d] && U[d] == sentinel);
                    owned[d] = 1; want[d] = u[p];
                }
                derive_u_pair(t, (int)e, blob.get(), off.w, U.get());
            }
    }
    for (int e = t.pairs; e < t.pairs + 256; ++e) derive_u_pair(t, e, blob.get(), off.w, U.get());      // threads past the last pair: nothing
    // every pair index was called, every float has its one owner (distinct, and as many as there are) and holds that pair's value: no other pair touched it
    CHECK(pairs == (size_t)t.pairs && floats == want_floats && memcmp(U.get(), want.get(), want_floats * sizeof(float)) == 0);
    printf("derived %s: %d sections, %d pairs, %zu floats: every float written once, by its own pair, with its transform\n", name, t.n, t.pairs, want_floats);
    return 0;
}

// the regions of the context's buffer: disjoint, back to back in this order, and together the buffer; form 2's one launch fills the two behind the 16-channel nets', form 3's the last three
static int check_regions() {
    const size_t t16 = derived_trunk16().floats, poly = derived_hardnet_poly().floats, f43 = derived_hardnet_f43().floats;
    const size_t c5 = F43C5::FLOATS;
    CHECK(DerivedU::AFFNET == 0 && DerivedU::ORINET == t16 && DerivedU::HARDNET == 2 * t16 && DerivedU::HARDNET_F43 == 2 * t16 + poly && DerivedU::HARDNET_C5 == 2 * t16 + poly + f43 &&
          DerivedU::FLOATS == 2 * t16 + poly + f43 + c5);
    CHECK(DerivedU::region(AFFNET_NET_AFFNET) == DerivedU::AFFNET && DerivedU::region(AFFNET_NET_ORINET) == DerivedU::ORINET && DerivedU::region(AFFNET_NET_HARDNET) == DerivedU::HARDNET);
    CHECK(derived_hardnet_form2().floats == poly + f43 && derived_hardnet_form3().floats == poly + f43 + c5);
    return 0;
}

int main() {
    for (int kind = 0; kind <= AFFNET_NET_AFFNET_FULLCONV; ++kind)
        if (check_kind(kind)) return 1;
    if (check_derived("AffNet", AFFNET_NET_AFFNET, derived_trunk16(), 5, 150016) || check_derived("OriNet", AFFNET_NET_ORINET, derived_trunk16(), 5, 150016) ||
        check_derived("HardNet polyphase", AFFNET_NET_HARDNET, derived_hardnet_poly(), 2, 256000) || check_derived("HardNet F(4x4, 3x3)", AFFNET_NET_HARDNET, derived_hardnet_f43(), 2, 184320) ||
        check_derived("HardNet form 2", AFFNET_NET_HARDNET, derived_hardnet_form2(), 4, 256000 + 184320) ||
        check_derived("HardNet form 3", AFFNET_NET_HARDNET, derived_hardnet_form3(), 5, 256000 + 184320 + 589824) || check_regions())
        return 1;
    return 0;
}
