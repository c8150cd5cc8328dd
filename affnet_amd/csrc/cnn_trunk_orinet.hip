// OriNet's six instantiations of cnn32_trunk_kernel (cnn_trunk.h).  The exact one reads derived weights (Wino16, weights_layout.h; aff_derive_u in front of every launch).
#include "cnn_trunk.h"

// by trunk form [phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check).
TrunkKernel aff_trunk_orinet(int form, bool stamps) { return trunk_unit<AFFNET_NET_ORINET, TRUNK_SPLIT2, TRUNK_SPLIT3, TRUNK_EXACT>(form, stamps); }
