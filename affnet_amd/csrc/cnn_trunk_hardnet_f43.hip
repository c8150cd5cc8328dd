// The exact HardNet trunk of descriptor form 2 (affnet_set_desc_form): cnn32_trunk_kernel<HardNet, 8, *, TRUNK_WINO_F43> (cnn_trunk.h) = form 1 with conv3 as Winograd
// F(4x4, 3x3); its weights from aff_derive_u (Poly32, F43 behind it).  A unit of its own for the reason cnn_trunk_hardnet_poly.hip is one: compiled beside
// the kernels it shares template instances with (conv0 .. conv2, conv4, conv5), the inliner's choices - and with them those kernels' code - change.
#include "cnn_trunk.h"

// by trunk form [phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check).
TrunkKernel aff_trunk_hardnet_f43(int form, bool stamps) { return trunk_unit<AFFNET_NET_HARDNET, TRUNK_WINO_F43>(form, stamps); }
