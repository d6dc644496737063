/* kfmi_inst_trace_seeds_mid_k1.hip -- traced seed and strand kernel instantiations for K=1, LAY_MID (see kfmi_kernels.h). */
#include "kfmi_kernels.h"

namespace kfmi {
KFMI_FOR_NB(KFMI_SEEDS_TRACE_INSTANTIATE, 1, LAY_MID)
}  // namespace kfmi
