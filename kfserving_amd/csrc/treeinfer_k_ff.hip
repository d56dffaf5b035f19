// Kernel instantiations for input type float, accumulator type float.
#include "treeinfer_dispatch.h"

namespace ti {
KernelFn kernels_ff(const KernelKey& k) { return select_types<float, float>(k); }
}  // namespace ti
