// Kernel instantiations of the categorical records (layout 11), every
// (input, accumulator) type pair: one unit, compiled beside treeinfer_k_*.hip.
#include "treeinfer_crec.h"
#include "treeinfer_dispatch.h"

namespace ti {
// the kernel is compiled per rule of the forest's categorical nodes (XGB); the
// LightGBM zero rule goes with LightGBM's categorical rule only (the host
// keeps a forest that pairs it with XGBoost's on layout 1)
template <typename XT, typename ACC>
static KernelFn crec_types(const KernelKey& k) {
  return with_k_zero<ACC>(k, [&k](auto KM, auto Z) -> KernelFn {
    return ilp_8_7_4(k.ilp, [&k](auto I) -> KernelFn {
      constexpr int KMAX = decltype(KM)::value, ILP = decltype(I)::value;
      constexpr bool ZERO = decltype(Z)::value;
      if (k.walk == Walk::CatRecordLgb) return crexplicit_predict_kernel<XT, ACC, KMAX, ZERO, ILP, false>;
      if constexpr (!ZERO) return crexplicit_predict_kernel<XT, ACC, KMAX, false, ILP, true>;
      return nullptr;
    });
  });
}

KernelFn kernels_crec(const KernelKey& k) {
  if (!k.x64) return k.acc64 ? crec_types<float, double>(k) : crec_types<float, float>(k);
  return k.acc64 ? crec_types<double, double>(k) : crec_types<double, float>(k);
}
}  // namespace ti
