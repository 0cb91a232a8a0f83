// fast_poly.hip -- the tolerance-mode (ROX_FAST_FP64) trace kernels of feature instance
// F_POLY (rox_math_fast.hpp, "tolerance mode"): every output mode (FULL packets: taken by the host where they pay).  One translation unit per
// instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(poly_fast, F_POLY | F_FAST)
}  // namespace rox
