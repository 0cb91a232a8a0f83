// inst_radial.hip -- the trace kernels of feature instance F_RADIAL (rox_device.hpp):
// one translation unit per instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(radial, F_RADIAL)
}  // namespace rox
