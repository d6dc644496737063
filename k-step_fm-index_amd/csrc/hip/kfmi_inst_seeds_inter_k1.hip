/* kfmi_inst_seeds_inter_k1.hip -- seed-search kernel instantiations for K=1, LAY_INTER (see kfmi_kernels.h). */
#include "kfmi_kernels.h"

namespace kfmi {
KFMI_FOR_NB(KFMI_SEEDS_INSTANTIATE, 1, LAY_INTER)
}  // namespace kfmi
