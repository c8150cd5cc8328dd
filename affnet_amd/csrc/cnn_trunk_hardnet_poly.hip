// The exact HardNet trunk of descriptor form 1 (affnet_set_desc_form): cnn32_trunk_kernel<HardNet, 8, *, TRUNK_WINO> (cnn_trunk.h), conv2 / conv4 as polyphase Winograd
// F(2x2, 2x2); their weights from aff_derive_u (Poly32).  A unit of its own: the form 0 kernels of cnn_trunk_hardnet.hip share template instances with this
// flow (conv1 / conv3 / conv5), and compiled together the inliner's choices - and with them the form 0 kernels' code - change.
#include "cnn_trunk.h"

// by trunk form [phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check).
TrunkKernel aff_trunk_hardnet_poly(int form, bool stamps) { return trunk_unit<AFFNET_NET_HARDNET, TRUNK_WINO>(form, stamps); }
