// Kernel instantiations of the categorical heap (layout 10), every
// (input, accumulator) type pair: one unit, compiled beside treeinfer_k_*.hip.
#include "treeinfer_cheap.h"

namespace ti {
template <bool XGB>
static CheapKernelFn cat_types(bool x64, bool acc64, int K, bool z) {
  if (!x64 && !acc64) return select_cheap<float, float, XGB>(K, z);
  if (!x64 && acc64) return select_cheap<float, double, XGB>(K, z);
  if (x64 && acc64) return select_cheap<double, double, XGB>(K, z);
  return select_cheap<double, float, XGB>(K, z);
}

CheapKernelFn kernels_cat(bool x64, bool acc64, int K, bool z, bool xgb) {
  return xgb ? cat_types<true>(x64, acc64, K, z) : cat_types<false>(x64, acc64, K, z);
}
}  // namespace ti
