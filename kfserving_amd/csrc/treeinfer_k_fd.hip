// Kernel instantiations for input type float, accumulator type double.
#include "treeinfer_dispatch.h"

namespace ti {
KernelFn kernels_fd(const KernelKey& k) { return select_types<float, double>(k); }
}  // namespace ti
