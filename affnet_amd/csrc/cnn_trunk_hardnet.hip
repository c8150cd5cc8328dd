// HardNet's six instantiations of cnn32_trunk_kernel (cnn_trunk.h).  (Tried and removed: 16-wave workgroups - slower.)
#include "cnn_trunk.h"

// by trunk form [phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check).
TrunkKernel aff_trunk_hardnet(int form, bool stamps) { return trunk_unit<AFFNET_NET_HARDNET, TRUNK_SPLIT2, TRUNK_SPLIT3, TRUNK_EXACT>(form, stamps); }
