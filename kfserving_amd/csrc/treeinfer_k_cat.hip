// Kernel instantiations of the categorical heap (layout 10), every
// (input, accumulator) type pair: one unit, compiled beside treeinfer_k_*.hip.
#include "treeinfer_cheap.h"
#include "treeinfer_dispatch.h"

namespace ti {
// the kernel is compiled per rule of the forest's categorical nodes (XGB)
template <typename XT, typename ACC>
static KernelFn cat_types(const KernelKey& k) {
  return with_k_zero<ACC>(k, [&k](auto KM, auto Z) -> KernelFn {
    return k.walk == Walk::CatHeapXgb
               ? cheap_predict_kernel<XT, ACC, decltype(KM)::value, decltype(Z)::value, true>
               : cheap_predict_kernel<XT, ACC, decltype(KM)::value, decltype(Z)::value, false>;
  });
}

KernelFn kernels_cat(const KernelKey& k) {
  if (!k.x64) return k.acc64 ? cat_types<float, double>(k) : cat_types<float, float>(k);
  return k.acc64 ? cat_types<double, double>(k) : cat_types<double, float>(k);
}
}  // namespace ti
