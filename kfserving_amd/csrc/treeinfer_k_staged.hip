// Kernel instantiations of TI_OUTPUT_STAGED's pass 2 (treeinfer_staged.h):
// float and double accumulators, scalar and vector leaves, KMAX = 16.  One
// unit, compiled beside treeinfer_k_*.hip.
#include "treeinfer_staged.h"
#include "treeinfer_dispatch.h"

namespace ti {
KernelFn kernels_staged(const KernelKey& k) {
  if (k.acc64) return k.vector_leaf ? staged_accum_kernel<double, true> : staged_accum_kernel<double, false>;
  return k.vector_leaf ? staged_accum_kernel<float, true> : staged_accum_kernel<float, false>;
}
}  // namespace ti
