// Kernel instantiations for input type double, accumulator type double.
#include "treeinfer_dispatch.h"

namespace ti {
KernelFn kernels_dd(const KernelKey& k) { return select_types<double, double>(k); }
}  // namespace ti
