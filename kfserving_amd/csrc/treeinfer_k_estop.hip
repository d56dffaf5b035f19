// Kernel instantiations of the round-checked walk of TI_OUTPUT_EARLY_STOP
// (treeinfer_estop.h), every (input, accumulator) type pair: one unit,
// compiled beside treeinfer_k_*.hip.
#include "treeinfer_estop.h"
#include "treeinfer_dispatch.h"

namespace ti {
template <typename XT, typename ACC>
static KernelFn estop_types(const KernelKey& k) {
  return with_k_zero<ACC>(k, [&k](auto KM, auto Z) -> KernelFn {
    constexpr int KMAX = decltype(KM)::value;
    constexpr bool ZERO = decltype(Z)::value;
    if (k.feat_lds) return estop_walk_kernel<XT, ACC, KMAX, true, ZERO>;
    return estop_walk_kernel<XT, ACC, KMAX, false, ZERO>;
  });
}

KernelFn kernels_estop(const KernelKey& k) {
  if (!k.x64) return k.acc64 ? estop_types<float, double>(k) : estop_types<float, float>(k);
  return k.acc64 ? estop_types<double, double>(k) : estop_types<double, float>(k);
}
}  // namespace ti
