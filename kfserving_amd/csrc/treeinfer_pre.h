// treeinfer_pre.h — pre-steps (ABI 9): the scaler and imputer steps of a
// sklearn Pipeline as one streaming pass in front of the walk (launch_pre in
// treeinfer.hip), and the whole of ti_pretransform_device.
//
// pre_steps_kernel reads the caller's [rows, F] tile (row_stride elements
// between rows, float32 or float64) and writes dense float32 [rows, F]: per
// element the S steps of treeinfer.h in order, each one float64 operation
// rounded to the input's element type, then the cast to float32.  It is
// memory-bound (12 or 8 bytes an element against at most 16 operations), so it
// is kept plain:
//
//   * the unit of work is an element of the dense output.  A lane's elements
//     are e, e + step, e + 2 step, ... with step = grid x block, so every wave
//     instruction reads 64 consecutive elements of a row (or of two rows where
//     a row ends) and writes 64 consecutive floats.  The grid is capped
//     (kPreMaxGrid) and strides over the rest, which also amortises the staging
//     below over many elements;
//   * a lane finds (row, column) of its first element with one 64-bit divide
//     and then only adds: the host passes step / F and step % F;
//   * the S x F constants and the S op codes are staged once per workgroup in
//     LDS when S * F * 8 fits kPreLdsBudget, else read from global memory (the
//     columns of consecutive lanes are consecutive, so those reads coalesce);
//   * an op code is the same for every lane: it is read once per step for the
//     kPreUnroll elements a lane has in flight and made a scalar, so the step
//     loop branches on SGPRs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "treeinfer.h"

namespace ti {

constexpr int kPreBlock = 256;                  // threads per workgroup
constexpr int kPreUnroll = 4;                   // elements a lane has in flight
constexpr int kPreMaxGrid = 2048;               // 256 CUs x 8 workgroups
constexpr size_t kPreLdsBudget = 32 * 1024;     // staged constants, bytes

struct PreArgs {
  const void* X;            // [n_rows, n_cols], row_stride elements between rows
  float* out;               // [n_rows, n_cols] dense
  const int32_t* ops;       // [S]
  const double* consts;     // [S * n_cols]
  int64_t row_stride;
  uint64_t total;           // n_rows * n_cols
  uint32_t n_cols;          // F
  int32_t n_steps;          // S
  uint32_t step;            // elements between two of a lane's: grid x block
  uint32_t step_rows;       // step / F
  uint32_t step_cols;       // step % F
};

// One step on one element.  The arithmetic is one IEEE float64 operation,
// rounded on its own whatever contraction mode the unit is compiled with, then
// rounded to XT; the division is the compiler's correctly rounded f64 division.
template <typename XT>
__device__ __forceinline__ XT pre_step(XT v, int op, double c) {
#pragma clang fp contract(off)
  const double w = (double)v;
  switch (op) {
    case TI_PRE_FILL_NAN: return v != v ? (XT)c : v;
    case TI_PRE_SUB: return (XT)(w - c);
    case TI_PRE_DIV: return (XT)(w / c);
    case TI_PRE_MUL: return (XT)(w * c);
    default: return (XT)(w + c);   // TI_PRE_ADD: ti_forest_create admits no other code
  }
}

template <typename XT, bool LDS>
__global__ void __launch_bounds__(kPreBlock) pre_steps_kernel(const PreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pre_smem[];
  const uint32_t F = a.n_cols;
  const int S = a.n_steps;
  const uint32_t tid = threadIdx.x;
  const double* cst = a.consts;
  const int32_t* ops = a.ops;
  if (LDS && S > 0) {
    double* lc = reinterpret_cast<double*>(pre_smem);
    int32_t* lo = reinterpret_cast<int32_t*>(pre_smem + (size_t)S * F * 8);
    const uint32_t n = (uint32_t)S * F;
    for (uint32_t i = tid; i < n; i += kPreBlock) lc[i] = a.consts[i];
    if (tid < (uint32_t)S) lo[tid] = a.ops[tid];
    __syncthreads();
    cst = lc;
    ops = lo;
  }
  const XT* X = static_cast<const XT*>(a.X);
  uint64_t e = (uint64_t)blockIdx.x * kPreBlock + tid;
  int64_t r = (int64_t)(e / F);               // the lane's one 64-bit divide
  uint32_t f = (uint32_t)(e - (uint64_t)r * F);
  while (e < a.total) {
    XT v[kPreUnroll];
    uint32_t col[kPreUnroll];
    uint64_t at[kPreUnroll];
#pragma unroll
    for (int u = 0; u < kPreUnroll; ++u) {
      at[u] = e;
      col[u] = f;                              // < F for dead elements too
      v[u] = e < a.total ? X[r * a.row_stride + f] : XT(0);
      e += a.step;
      r += a.step_rows;
      f += a.step_cols;
      if (f >= F) {
        f -= F;
        ++r;
      }
    }
    for (int s = 0; s < S; ++s) {
      const int op = __builtin_amdgcn_readfirstlane(ops[s]);
      const double* cs = cst + (size_t)s * F;
#pragma unroll
      for (int u = 0; u < kPreUnroll; ++u) v[u] = pre_step<XT>(v[u], op, cs[col[u]]);
    }
#pragma unroll
    for (int u = 0; u < kPreUnroll; ++u)
      if (at[u] < a.total) a.out[at[u]] = (float)v[u];
  }
}

using PreFn = void (*)(PreArgs);

inline PreFn select_pre(bool x64, bool lds) {
  if (x64) return lds ? pre_steps_kernel<double, true> : pre_steps_kernel<double, false>;
  return lds ? pre_steps_kernel<float, true> : pre_steps_kernel<float, false>;
}

}  // namespace ti
