// The transformed weights that are no blob sections (weights_layout.h: derived sections, DerivedU): the one kernel that derives them from a blob's taps, the
// context's buffer and the launcher.  A unit of its own: beside the trunk kernels it would take part in the inliner's choices for them.
#include "common.h"

// One thread per (cin, cout) pair of the table's sections: derive_u_pair (weights_layout.h), which the host check runs as well (pack_check.cpp)
__global__ __launch_bounds__(256) void derive_u_kernel(const float* __restrict__ packed, NetOffsets off, DerivedTable t, float* __restrict__ U) {
    derive_u_pair(t, blockIdx.x * 256 + threadIdx.x, packed, off.w, U);
}

// Allocated on first use; affnet_graph_capture_extract calls this before the capture begins (no allocation inside a capture).
int aff_derived_u_ensure(affnet_ctx* ctx) {
    if (ctx->derived_u) return AFFNET_OK;
    AFF_HIP(ctx, hipMalloc((void**)&ctx->derived_u, (size_t)DerivedU::FLOATS * sizeof(float)));
    return AFFNET_OK;
}

// the sections the exact trunk (kind, form) reads; n == 0: none
static DerivedTable table_of(int kind, int form) {
    if (kind == AFFNET_NET_HARDNET) return form == TRUNK_WINO ? derived_hardnet_poly() : (form == TRUNK_WINO_F43 ? derived_hardnet_form2() : (form == TRUNK_WINO_F43_C5 || form == TRUNK_WINO_F43_C1 ? derived_hardnet_form3() : DerivedTable{}));
    const bool wino = kind == AFFNET_NET_ORINET ? form == TRUNK_EXACT : (form == TRUNK_WINO || form == TRUNK_WINO_POLY);
    return wino ? derived_trunk16() : DerivedTable{};
}

// On the launch stream, ONE launch of a thread per pair (7936 threads, 286 KB read, 600 KB written for a 16-channel net; 15360, 0.55 MB, 1.8 MB for HardNet form 2; 31744, 1.1 MB, 4.1 MB for form 3).
// In front of EVERY launch of a trunk that reads them, so that a blob rewritten in place (load_state_dict into the same device buffer) can never meet stale weights, eagerly or in a replayed graph.
int aff_derive_u(affnet_ctx* ctx, int kind, int form, const float* packed, const NetLayout& L, hipStream_t st, const float** region) {
    *region = nullptr;
    const DerivedTable t = table_of(kind, form);
    if (t.n == 0) return AFFNET_OK;
    const int rc = aff_derived_u_ensure(ctx);
    if (rc) return rc;
    float* dst = ctx->derived_u + DerivedU::region(kind);
    hipLaunchKernelGGL(derive_u_kernel, dim3(t.pairs / 256), dim3(256), 0, st, packed, to_offsets(L), t, dst);
    AFF_LAUNCH_CHECK(ctx);
    *region = dst;
    return AFFNET_OK;
}
