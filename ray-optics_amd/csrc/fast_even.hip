// fast_even.hip -- the tolerance-mode (ROX_FAST_FP64) trace kernels of feature instance
// F_EVEN (rox_math_fast.hpp, "tolerance mode"): every output mode (FULL packets: taken by the host where they pay).  One translation unit per
// instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(even_fast, F_EVEN | F_FAST)
}  // namespace rox
