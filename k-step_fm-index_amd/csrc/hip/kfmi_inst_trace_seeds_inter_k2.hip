/* kfmi_inst_trace_seeds_inter_k2.hip -- traced seed and strand kernel instantiations for K=2, LAY_INTER (see kfmi_kernels.h). */
#include "kfmi_kernels.h"

namespace kfmi {
KFMI_FOR_NB(KFMI_SEEDS_TRACE_INSTANTIATE, 2, LAY_INTER)
}  // namespace kfmi
