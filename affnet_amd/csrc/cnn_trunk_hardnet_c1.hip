// The exact HardNet trunk of descriptor form 4 (affnet_set_desc_form): cnn32_trunk_kernel<HardNet, 8, *, TRUNK_WINO_F43_C1> (cnn_trunk.h) = form 3 with conv0 + conv1 streamed
// over conv1's K and conv1 as Winograd F(4x4, 3x3); conv5 follows in hardnet_conv5_f43.hip as in form 3.  A unit of its own for the reason cnn_trunk_hardnet_c5.hip is one:
// compiled beside the kernels it shares template instances with (conv2 .. conv4), the inliner's choices - and with them those kernels' code - change.
#include "cnn_trunk.h"

// by trunk form [phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check).
TrunkKernel aff_trunk_hardnet_c1(int form, bool stamps) { return trunk_unit<AFFNET_NET_HARDNET, TRUNK_WINO_F43_C1>(form, stamps); }
