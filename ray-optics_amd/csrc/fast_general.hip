// fast_general.hip -- the tolerance-mode (ROX_FAST_FP64) trace kernels of feature instance
// F_ALL (rox_math_fast.hpp, "tolerance mode"): every output mode (FULL packets: taken by the host where they pay).  One translation unit per
// instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(general_fast, F_ALL | F_FAST)
}  // namespace rox
