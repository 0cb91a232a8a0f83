// inst_poly.hip -- the trace kernels of feature instance F_POLY (rox_device.hpp):
// one translation unit per instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(poly, F_POLY)
}  // namespace rox
