/* kfmi_inst_seeds_mid_k1.hip -- seed-search kernel instantiations for K=1, LAY_MID (see kfmi_kernels.h). */
#include "kfmi_kernels.h"

namespace kfmi {
KFMI_FOR_NB(KFMI_SEEDS_INSTANTIATE, 1, LAY_MID)
}  // namespace kfmi
