// AffNet's eight instantiations of cnn32_trunk_kernel (cnn_trunk.h): six as every net has them, two of the exact flow with Winograd conv1 / conv3 / conv5.  (Tried and removed: two AffNet patches per persistent 16-wave workgroup in anti-phase - correct
// but 8 % slower, the small-tile loops reach 85-90 % of the pipe rate with two waves per SIMD.)
#include "cnn_trunk.h"

// [exact, three bf16 terms, two fp16 terms][phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check)
TrunkKernel aff_trunk_affnet(int arith_index, bool stamps) {
    static const TrunkKernel k[3][2] = {{cnn32_trunk_kernel<AFFNET_NET_AFFNET, 8, false>, cnn32_trunk_kernel<AFFNET_NET_AFFNET, 8, true>},
                                        {cnn32_trunk_kernel<AFFNET_NET_AFFNET, 8, false, 3>, cnn32_trunk_kernel<AFFNET_NET_AFFNET, 8, true, 3>},
                                        {cnn32_trunk_kernel<AFFNET_NET_AFFNET, 8, false, 2>, cnn32_trunk_kernel<AFFNET_NET_AFFNET, 8, true, 2>}};
    return k[arith_index][stamps];
}

// Exact fp32 with conv1 / conv3 / conv5 as Winograd F(2x2, 3x3) (U from aff_wino_derive_u), the head from conv5's fragments: what the fused shape pass runs on every row in shape form 1
TrunkKernel aff_trunk_affnet_wino(bool stamps) {
    return stamps ? cnn32_trunk_kernel<AFFNET_NET_AFFNET, 8, true, 1> : cnn32_trunk_kernel<AFFNET_NET_AFFNET, 8, false, 1>;
}
