// inst_lean.hip -- the trace kernels of feature instance 0 (rox_device.hpp):
// one translation unit per instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(lean, 0)
}  // namespace rox
