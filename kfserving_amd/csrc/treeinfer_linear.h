// treeinfer_linear.h — linear leaves (LightGBM linear_tree, ABI 6): the second
// of the two stream-ordered passes of launch_linear (treeinfer.hip).
//
// Pass 1 is the forest's own walk with TI_OUTPUT_LEAF into a [rows, T] int32
// scratch: whichever layout ti_forest_create picked keeps walking rank-binned
// features.  Pass 2, here, holds what those layouts do not: the raw feature
// values.  One lane per row; the tile's features are staged into LDS as
// [F][R] by stage_features (zero-mapped, columns >= n_cols NaN) when they fit,
// else read from the row in HBM by the explicit kernel's rule.  For each tree
// in order the lane looks up its leaf's record, runs the term loop of
// treeinfer.h in float64 and adds the result into its group's sum, so the
// margins are the library's sequential sums bit for bit.  The epilogue is the
// walk kernels' init_acc / finish_row.
//
// Leaf ids are read kLinTC trees at a time: the [R][kLinTC] block of the
// scratch is loaded coalesced (consecutive lanes read consecutive trees of a
// row, 128 B a row) and transposed through LDS with a row pitch of kLinTC + 1
// words, so the per-lane reads that follow (lane r, word r * 33 + j) fall in
// distinct banks.
#pragma once

#include "treeinfer_kernels.h"

namespace ti {

constexpr int kLinTC = 32;             // trees per leaf-id chunk
constexpr int kLinPitch = kLinTC + 1;  // words per row of the transposed chunk

// One term of a leaf's linear model: a single 16-byte load.
struct LinTerm {
  double coeff;
  uint32_t feature;
  uint32_t pad;
};
static_assert(sizeof(LinTerm) == 16, "a term is one global_load_dwordx4");

// One leaf's record: two 16-byte loads.
struct LinLeaf {
  double lconst;     // leaf_const
  double fallback;   // leaf_value: what the leaf adds when a term's feature is NaN
  uint32_t begin;    // first term
  uint32_t count;    // terms
  uint32_t pad[2];
};
static_assert(sizeof(LinLeaf) == 32, "a leaf record is two global_load_dwordx4");

// The linear pass's own arguments (beside the walk kernels' KArgs, which the
// shared prologue and epilogue read and which stays as it is).
struct LinArgs {
  const int32_t* leaf_ids;    // [n_rows][T] pass 1's output for the rows of this launch
  const LinLeaf* leaves;      // [sum of leaves]
  const LinTerm* terms;       // [M]
  const int64_t* leaf_base;   // [T] first record of each tree; a tree's records are
                              //     indexed by the library leaf id (0 .. L-1)
};

// out + c * v with the product rounded before the sum, whatever contraction
// mode the unit is compiled with.
__device__ __forceinline__ double lin_mul_add(double out, double c, double v) {
#pragma clang fp contract(off)
  const double p = c * v;
  return out + p;
}

__device__ __forceinline__ LinTerm load_term(const LinTerm* p) {
  const u32x4 w = *reinterpret_cast<const u32x4*>(p);
  LinTerm t;
  t.coeff = __hiloint2double((int)w.y, (int)w.x);
  t.feature = w.z;
  t.pad = 0;
  return t;
}

template <typename XT, int KMAX, bool FEAT_LDS>
__global__ void __launch_bounds__(256) linear_leaf_kernel(const KArgs a, const LinArgs la) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = blockDim.x;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int64_t row = row0 + tid;
  const bool live = row < a.n_rows;
  const int64_t left_rows = a.n_rows - row0;
  const int rows_here = left_rows < R ? (int)left_rows : R;
  XT* feat = reinterpret_cast<XT*>(smem);
  const XT* xrow = static_cast<const XT*>(a.X) + (live ? row : a.n_rows - 1) * a.row_stride;
  const size_t feat_bytes = FEAT_LDS ? align16((size_t)a.n_features * R * sizeof(XT)) : 0;
  if (FEAT_LDS) {
    volatile int* flag = reinterpret_cast<volatile int*>(smem + feat_bytes);
    stage_features<XT>(feat, flag, a, row0, R, tid);   // ends in a barrier
  }
  int32_t* tile = reinterpret_cast<int32_t*>(smem + feat_bytes + 16);   // [R][kLinPitch]
  const int T = a.n_trees;

  double acc[KMAX];
  init_acc(acc, a);

  for (int t0 = 0; t0 < T; t0 += kLinTC) {
    const int tc = T - t0 < kLinTC ? T - t0 : kLinTC;
    if (t0 > 0) __syncthreads();   // the previous chunk has been read
    // coalesced [rows_here][tc] block -> transposed tile
    const int32_t* src = la.leaf_ids + row0 * (int64_t)T + t0;
    for (int e = tid; e < rows_here * kLinTC; e += R) {
      const int r = e / kLinTC;
      const int j = e - r * kLinTC;
      if (j < tc) tile[r * kLinPitch + j] = src[(int64_t)r * T + j];
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < tc; ++j) {
        const int t = t0 + j;
        const int32_t leaf = tile[tid * kLinPitch + j];
        const LinLeaf* lp = la.leaves + la.leaf_base[t] + leaf;
        const u32x4 w0 = reinterpret_cast<const u32x4*>(lp)[0];
        const u32x4 w1 = reinterpret_cast<const u32x4*>(lp)[1];
        double out = __hiloint2double((int)w0.y, (int)w0.x);
        const double fallback = __hiloint2double((int)w0.w, (int)w0.z);
        const LinTerm* tp = la.terms + w1.x;
        const uint32_t n = w1.y;
        bool nan_found = false;
        for (uint32_t i = 0; i < n; ++i) {
          const LinTerm term = load_term(tp + i);
          XT x;
          if (FEAT_LDS) {
            x = feat[term.feature * R + tid];
          } else {
            x = (int)term.feature < a.n_cols ? zero_map(xrow[term.feature], a.lgb_zero_map)
                                             : nan_value<XT>();
          }
          const double v = (double)x;
          nan_found |= v != v;
          out = lin_mul_add(out, term.coeff, v);
        }
        const double val = nan_found ? fallback : out;   // the partial sum is discarded
        if (KMAX == 1) {
          acc[0] += val;
        } else {
          const int g = a.tree_group[t];
#pragma unroll
          for (int k = 0; k < KMAX; ++k) acc[k] = (k == g) ? acc[k] + val : acc[k];
        }
      }
    }
  }
  if (!live) return;
  finish_row<double, KMAX>(acc, a, row);
}

using LinearFn = void (*)(KArgs, LinArgs);

template <typename XT>
LinearFn select_linear(int K, bool feat_lds) {
  if (K == 1) return feat_lds ? linear_leaf_kernel<XT, 1, true> : linear_leaf_kernel<XT, 1, false>;
  if (K <= 4) return feat_lds ? linear_leaf_kernel<XT, 4, true> : linear_leaf_kernel<XT, 4, false>;
  return feat_lds ? linear_leaf_kernel<XT, 16, true> : linear_leaf_kernel<XT, 16, false>;
}

}  // namespace ti
