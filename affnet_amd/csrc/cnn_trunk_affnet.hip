// AffNet's eight instantiations of cnn32_trunk_kernel (cnn_trunk.h): six as every net has them, two of the exact flow with Winograd conv1 / conv3 / conv5.  (Tried and removed: two AffNet patches per persistent 16-wave workgroup in anti-phase - correct
// but 8 % slower, the small-tile loops reach 85-90 % of the pipe rate with two waves per SIMD.)
#include "cnn_trunk.h"

// by trunk form [phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check).  TRUNK_WINO: conv1 / conv3 / conv5 as Winograd F(2x2, 3x3) (U from aff_derive_u), the head from conv5's fragments - what the fused shape pass runs on every row in shape form 1
TrunkKernel aff_trunk_affnet(int form, bool stamps) { return trunk_unit<AFFNET_NET_AFFNET, TRUNK_WINO, TRUNK_SPLIT2, TRUNK_SPLIT3, TRUNK_EXACT>(form, stamps); }
