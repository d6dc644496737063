/* kfmi_inst_trace_inter_k1.hip -- traced task kernel instantiations for K=1, LAY_INTER (see kfmi_kernels.h). */
#include "kfmi_kernels.h"

namespace kfmi {
KFMI_FOR_NB(KFMI_TRACE_INSTANTIATE, 1, LAY_INTER)
}  // namespace kfmi
