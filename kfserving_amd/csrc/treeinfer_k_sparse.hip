// Kernel instantiations of the CSR walk (ti_predict_csr), every (input,
// accumulator) type pair: one unit, compiled beside treeinfer_k_*.hip.
#include "treeinfer_sparse.h"
#include "treeinfer_dispatch.h"

namespace ti {
template <typename XT, typename ACC>
static KernelFn sparse_types(const KernelKey& k) {
  return with_k_zero<ACC>(k, [&k](auto KM, auto Z) -> KernelFn {
    constexpr int KMAX = decltype(KM)::value;
    constexpr bool ZERO = decltype(Z)::value;
    if (k.walk == Walk::SparseSearch) return sparse_explicit_predict_kernel<XT, ACC, KMAX, ZERO, true>;
    return sparse_explicit_predict_kernel<XT, ACC, KMAX, ZERO, false>;
  });
}

KernelFn kernels_sparse(const KernelKey& k) {
  if (!k.x64) return k.acc64 ? sparse_types<float, double>(k) : sparse_types<float, float>(k);
  return k.acc64 ? sparse_types<double, double>(k) : sparse_types<double, float>(k);
}
}  // namespace ti
