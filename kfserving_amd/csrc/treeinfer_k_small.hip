// Kernel instantiations of the tree-parallel small-batch walk
// (TI_OPT_SMALL_BATCH_ROWS), every (input, accumulator) type pair: one unit,
// compiled beside treeinfer_k_*.hip.
#include "treeinfer_small.h"
#include "treeinfer_dispatch.h"

namespace ti {
template <typename XT, typename ACC>
static KernelFn small_types(const KernelKey& k) {
  return with_k_zero<ACC>(k, [&k](auto KM, auto Z) -> KernelFn {
    constexpr int KMAX = decltype(KM)::value;
    constexpr bool ZERO = decltype(Z)::value;
    if (k.feat_lds) return tree_lanes_predict_kernel<XT, ACC, KMAX, true, ZERO>;
    return tree_lanes_predict_kernel<XT, ACC, KMAX, false, ZERO>;
  });
}

KernelFn kernels_small(const KernelKey& k) {
  if (!k.x64) return k.acc64 ? small_types<float, double>(k) : small_types<float, float>(k);
  return k.acc64 ? small_types<double, double>(k) : small_types<double, float>(k);
}
}  // namespace ti
