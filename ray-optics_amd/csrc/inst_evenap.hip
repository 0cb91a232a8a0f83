// inst_evenap.hip -- the trace kernels of feature instance F_EVEN | F_APLIST (rox_device.hpp):
// even aspheres + clear-aperture lists, i.e. a Zemax import with EVENASPH surfaces.
// One translation unit per instance so that the instances compile in parallel.
#include "rox_device.hpp"

namespace rox {
ROX_TRACE_INSTANCE(evenap, F_EVEN | F_APLIST)
}  // namespace rox
