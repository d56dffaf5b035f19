// treeinfer_dispatch.h — kernel selection across the translation units.  Each
// treeinfer_k_<x><a>.hip instantiates every kernel of one (input type,
// accumulator type) pair and treeinfer_k_cat.hip the categorical heap's for
// all four pairs, so the five compile in parallel.
//
// The host names what it launches with a KernelKey; ti::select(key) is the one
// way from a key to a kernel.  Each rule that turns a runtime value into a
// template argument (K buckets, the zero rule, ILP rounding, prefetch depth,
// group count) is written once below, at the walk it belongs to.
#pragma once

#include <type_traits>

#include "treeinfer_kernels.h"

namespace ti {

using KernelFn = void (*)(KArgs);

// What a launch walks.  The number is the public layout (ti_forest_info) that
// reaches it; 2, 4 and 5 were retired in round 3.
enum class Walk {
  Heap,             // 0: float heap                      heap_predict_kernel
  Explicit,         // 1: float explicit                  explicit_predict_kernel
  BinHeap,          // 3: binned heap, indexed walk       bheap_predict_kernel
  BinHeapFixed,     // 3: binned heap, fixed-layout walk  bheap_fix_kernel
  Record,           // 6: record explicit                 rexplicit_predict_kernel
  StagedRecord,     // 7: staged record explicit          lexplicit_predict_kernel
  HeapTopRecord,    // 8: heap top + record bottom        hexplicit_predict_kernel
  HeapTopStaged,    // 9: heap top + staged record bottom texplicit_predict_kernel
  BottomU8,         // 9: its compact u8 bottom           t8explicit_predict_kernel
  BottomU16,        // 9: its compact u16 bottom          t16explicit_predict_kernel
  BottomU16Split,   // 9: the u16 bottom, two lanes a row t16split_predict_kernel
  CatHeapXgb,       // 10: categorical heap, XGBoost's rule   cheap_predict_kernel
  CatHeapLgb,       // 10: categorical heap, LightGBM's rule  (treeinfer_cheap.h)
};

struct KernelKey {
  Walk walk;
  bool x64, acc64;   // float64 input / sums (else float32)
  int K;             // output groups
  bool feat_lds;     // Heap, Explicit: feature image in LDS
  bool zero_rule;    // LightGBM zero rule (no binned heap walk has one)
  bool bins16;       // BinHeap, BinHeapFixed, HeapTopStaged: u16 bins (else u8)
  int ilp;           // record walks and bottoms: trees a lane walks at once
  int prefetch;      // BinHeap: prefetch depth
  int groups;        // BinHeapFixed: groups of 4 trees a stage (NG)
};

// A rule calls `f` with the template argument it chose, as an
// integral_constant: f(Int<8>{}) -> kernel<..., 8>.
template <int V>
using Int = std::integral_constant<int, V>;

// K buckets to 1 / 4 / 16.  The LightGBM zero rule selects a ZERO kernel only
// when the sums are float64; with float32 sums it is ignored.
template <typename ACC, typename F>
KernelFn with_k_zero(const KernelKey& k, F f) {
  if constexpr (sizeof(ACC) == 8) {
    if (k.zero_rule)
      return k.K == 1 ? f(Int<1>{}, std::true_type{})
           : k.K <= 4 ? f(Int<4>{}, std::true_type{}) : f(Int<16>{}, std::true_type{});
  }
  return k.K == 1 ? f(Int<1>{}, std::false_type{})
       : k.K <= 4 ? f(Int<4>{}, std::false_type{}) : f(Int<16>{}, std::false_type{});
}

// Tree ILP rounding.  Records take 16 / 8 / 4; the staged walks (about a
// stage's trees) 8 / 7 / 4; the heap top and the u16 bottom 8 / 4, so 7 gives 4.
template <typename F>
KernelFn ilp_16_8_4(int ilp, F f) {
  return ilp >= 16 ? f(Int<16>{}) : ilp >= 8 ? f(Int<8>{}) : f(Int<4>{});
}
template <typename F>
KernelFn ilp_8_7_4(int ilp, F f) {
  return ilp >= 8 ? f(Int<8>{}) : ilp == 7 ? f(Int<7>{}) : f(Int<4>{});
}
template <typename F>
KernelFn ilp_8_4(int ilp, F f) {
  return ilp >= 8 ? f(Int<8>{}) : f(Int<4>{});
}

template <typename XT, typename ACC, int KMAX, bool ZERO>
KernelFn select_walk(const KernelKey& k) {
  switch (k.walk) {
    case Walk::Heap:
      return k.feat_lds ? heap_predict_kernel<XT, ACC, KMAX, true, ZERO>
                        : heap_predict_kernel<XT, ACC, KMAX, false, ZERO>;
    case Walk::Explicit:
      return k.feat_lds ? explicit_predict_kernel<XT, ACC, KMAX, true, ZERO>
                        : explicit_predict_kernel<XT, ACC, KMAX, false, ZERO>;
    case Walk::BinHeap:   // prefetch depth 4 up to 4, else 8
      if (k.bins16) return k.prefetch <= 4 ? bheap_predict_kernel<XT, ACC, KMAX, true, 4>
                                           : bheap_predict_kernel<XT, ACC, KMAX, true, 8>;
      return k.prefetch <= 4 ? bheap_predict_kernel<XT, ACC, KMAX, false, 4>
                             : bheap_predict_kernel<XT, ACC, KMAX, false, 8>;
    case Walk::BinHeapFixed:   // float X, float sums only; NG 2 from 2 up, else 1
      if constexpr (sizeof(XT) == 4 && sizeof(ACC) == 4) {
        if (k.bins16) return k.groups >= 2 ? bheap_fix_kernel<XT, KMAX, true, 2>
                                           : bheap_fix_kernel<XT, KMAX, true, 1>;
        return k.groups >= 2 ? bheap_fix_kernel<XT, KMAX, false, 2>
                             : bheap_fix_kernel<XT, KMAX, false, 1>;
      }
      return nullptr;
    case Walk::Record:
      return ilp_16_8_4(k.ilp, [](auto I) -> KernelFn {
        return rexplicit_predict_kernel<XT, ACC, KMAX, ZERO, decltype(I)::value>;
      });
    case Walk::StagedRecord:
      return ilp_8_7_4(k.ilp, [](auto I) -> KernelFn {
        return lexplicit_predict_kernel<XT, ACC, KMAX, ZERO, decltype(I)::value>;
      });
    case Walk::HeapTopRecord:
      return ilp_8_4(k.ilp, [](auto I) -> KernelFn {
        return hexplicit_predict_kernel<XT, ACC, KMAX, ZERO, decltype(I)::value>;
      });
    case Walk::HeapTopStaged:   // last argument B8: u8 bins
      return ilp_8_7_4(k.ilp, [&k](auto I) -> KernelFn {
        return k.bins16 ? texplicit_predict_kernel<XT, ACC, KMAX, ZERO, decltype(I)::value, false>
                        : texplicit_predict_kernel<XT, ACC, KMAX, ZERO, decltype(I)::value, true>;
      });
    case Walk::BottomU8:
      return ilp_8_7_4(k.ilp, [](auto I) -> KernelFn {
        return t8explicit_predict_kernel<XT, ACC, KMAX, ZERO, decltype(I)::value>;
      });
    case Walk::BottomU16:
      return ilp_8_4(k.ilp, [](auto I) -> KernelFn {
        return t16explicit_predict_kernel<XT, ACC, KMAX, ZERO, decltype(I)::value>;
      });
    case Walk::BottomU16Split:   // always 4 trees a lane (8 a group)
      return t16split_predict_kernel<XT, ACC, KMAX, ZERO, 4>;
    case Walk::CatHeapXgb:
    case Walk::CatHeapLgb:
      break;   // kernels_cat
  }
  return nullptr;
}

template <typename XT, typename ACC>
KernelFn select_types(const KernelKey& k) {
  return with_k_zero<ACC>(k, [&k](auto KM, auto Z) -> KernelFn {
    return select_walk<XT, ACC, decltype(KM)::value, decltype(Z)::value>(k);
  });
}

KernelFn kernels_ff(const KernelKey& k);    // float X, float acc
KernelFn kernels_fd(const KernelKey& k);    // float X, double acc
KernelFn kernels_dd(const KernelKey& k);    // double X, double acc
KernelFn kernels_df(const KernelKey& k);    // double X, float acc
KernelFn kernels_cat(const KernelKey& k);   // the categorical heap, every pair

inline KernelFn select(const KernelKey& k) {
  if (k.walk == Walk::CatHeapXgb || k.walk == Walk::CatHeapLgb) return kernels_cat(k);
  if (!k.x64) return k.acc64 ? kernels_fd(k) : kernels_ff(k);
  return k.acc64 ? kernels_dd(k) : kernels_df(k);
}

}  // namespace ti
