// The exact HardNet trunk of descriptor form 3 (affnet_set_desc_form): cnn32_trunk_kernel<HardNet, 8, *, TRUNK_WINO_F43_C5> (cnn_trunk.h) = form 2 up to conv4's loop, conv4's
// tensor to HBM; conv5 follows in hardnet_conv5_f43.hip.  A unit of its own for the reason cnn_trunk_hardnet_poly.hip is one: compiled beside the kernels it shares template
// instances with (conv0 .. conv4), the inliner's choices - and with them those kernels' code - change.
#include "cnn_trunk.h"

// by trunk form [phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check).
TrunkKernel aff_trunk_hardnet_c5(int form, bool stamps) { return trunk_unit<AFFNET_NET_HARDNET, TRUNK_WINO_F43_C5>(form, stamps); }
