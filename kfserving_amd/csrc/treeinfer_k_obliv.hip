// Kernel instantiations of the oblivious trees (layout 12), every (input,
// accumulator) type pair: one unit, compiled beside treeinfer_k_*.hip.
#include "treeinfer_obliv.h"
#include "treeinfer_dispatch.h"

namespace ti {
// GATHER is compiled in only for a forest that has a tree too large to stage
// (Walk::ObliviousGather); an oblivious forest has no LightGBM zero rule
template <typename XT, typename ACC>
static KernelFn obliv_types(const KernelKey& k) {
  return with_k_zero<ACC>(k, [&k](auto KM, auto Z) -> KernelFn {
    constexpr int KMAX = decltype(KM)::value;
    if constexpr (decltype(Z)::value) return nullptr;
    if (k.walk == Walk::ObliviousGather) return oblivious_predict_kernel<XT, ACC, KMAX, true>;
    return oblivious_predict_kernel<XT, ACC, KMAX, false>;
  });
}

KernelFn kernels_obliv(const KernelKey& k) {
  if (!k.x64) return k.acc64 ? obliv_types<float, double>(k) : obliv_types<float, float>(k);
  return k.acc64 ? obliv_types<double, double>(k) : obliv_types<double, float>(k);
}
}  // namespace ti
