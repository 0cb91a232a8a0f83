// inst_general.hip -- the trace kernels of feature instance F_ALL (rox_device.hpp):
// one translation unit per instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(general, F_ALL)
}  // namespace rox
