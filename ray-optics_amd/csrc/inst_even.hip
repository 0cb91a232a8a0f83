// inst_even.hip -- the trace kernels of feature instance F_EVEN (rox_device.hpp):
// one translation unit per instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(even, F_EVEN)
}  // namespace rox
