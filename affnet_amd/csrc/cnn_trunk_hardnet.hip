// HardNet's six instantiations of cnn32_trunk_kernel (cnn_trunk.h).  (Tried and removed: 16-wave workgroups - slower.)
#include "cnn_trunk.h"

// [exact, three bf16 terms, two fp16 terms][phase stamps]; stamps = dbg_time or a layer dump (exact mode only, see cnn_check)
TrunkKernel aff_trunk_hardnet(int arith_index, bool stamps) {
    static const TrunkKernel k[3][2] = {{cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, false>, cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, true>},
                                        {cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, false, 3>, cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, true, 3>},
                                        {cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, false, 2>, cnn32_trunk_kernel<AFFNET_NET_HARDNET, 8, true, 2>}};
    return k[arith_index][stamps];
}
