// Kernel instantiations for input type double, accumulator type float.
#include "treeinfer_dispatch.h"

namespace ti {
KernelFn kernels_df(const KernelKey& k) { return select_types<double, float>(k); }
}  // namespace ti
