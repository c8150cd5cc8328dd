// The first AffNet trunk of shape form 2 (affnet_set_shape_form): cnn32_trunk_kernel<AffNet, 8, *, TRUNK_WINO_POLY> (cnn_trunk.h) - the Winograd trunk of form 1 (conv1 / conv3 / conv5 as
// F(2x2, 3x3), the head from conv5's fragments) with conv2 / conv4 as polyphase Winograd F(2x2, 2x2) (cnn_mfma.h: conv3x3_poly16_mfma_rows); U of all five layers from
// aff_derive_u.  A unit of its own, as the HardNet forms are: compiled next to the kernels of cnn_trunk_affnet.hip it would change their code, and form 1's layer 4 is
// pinned bit for bit.
#include "cnn_trunk.h"

// by trunk form [phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check).
TrunkKernel aff_trunk_affnet_poly(int form, bool stamps) { return trunk_unit<AFFNET_NET_AFFNET, TRUNK_WINO_POLY>(form, stamps); }
