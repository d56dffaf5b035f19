// treeinfer_small.h -- the tree-parallel walk of small batches
// (TI_OPT_SMALL_BATCH_ROWS).
//
// Every other walk gives a lane a row and streams the forest past it; a batch
// of a few rows then fills one workgroup, which walks the T trees one after
// another on one CU.  Here the split is turned round: a workgroup owns ONE row
// and a lane owns one tree.  The block is min(1024, T rounded up to 64) lanes;
// pass p walks the trees [p * block, (p + 1) * block), lane i tree p * block + i.
//
//   1. the row goes to LDS once as XT feat[F] (coalesced, zero_map applied, a
//      column >= n_cols NaN); FEAT_LDS = false reads it from global memory, where
//      every lane hits the same few lines;
//   2. a lane walks its tree over the layout-1 nodes in global memory (the float
//      explicit kernel's step: go_left / cat_left / cat_left_xgb) and writes the
//      leaf it reached to leaf_of[i] -- it adds nothing;
//   3. the pass's leaf values are gathered into LDS by the whole workgroup
//      (independent loads, kSmallValBytes at a time), and lane k < KMAX replays
//      the adds of output k over them in tree order: add_leaf's arithmetic on
//      one column.  Columns never mix before finish_row, so each output sees the
//      adds explicit_predict_kernel gives it, in its order: the same bits.
//   4. after the last pass lane 0 collects the KMAX sums and runs finish_row.
//
// TI_OUTPUT_LEAF stops after step 2 and writes the pass's ids, coalesced.
#pragma once

#include "treeinfer_kernels.h"

namespace ti {

constexpr int kSmallMaxBlock = 1024;
constexpr size_t kSmallValBytes = 16 * 1024;   // leaf values gathered per replay step

// LDS: [feat: F XT | leaf_of: block i32 | grp: block i32 | val: kSmallValBytes |
// sums: kMaxGroups doubles].  feat_bytes = 0 without the LDS row.
__host__ __device__ constexpr size_t small_feat_bytes(size_t F, size_t xs) {
  return (F * xs + 15) & ~size_t(15);
}
__host__ __device__ constexpr size_t small_lds_bytes(size_t feat_bytes, size_t block) {
  return feat_bytes + 2 * block * 4 + kSmallValBytes + kMaxGroups * 8;
}

template <typename XT, typename ACC, int KMAX, bool FEAT_LDS, bool ZERO>
__global__ void __launch_bounds__(kSmallMaxBlock) tree_lanes_predict_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int B = blockDim.x;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;   // grid = n_rows
  const int F = a.n_features;
  const size_t fb = FEAT_LDS ? small_feat_bytes(F, sizeof(XT)) : 0;
  XT* feat = reinterpret_cast<XT*>(smem);
  int32_t* leaf_of = reinterpret_cast<int32_t*>(smem + fb);
  int32_t* grp = leaf_of + B;
  ACC* val = reinterpret_cast<ACC*>(smem + fb + (size_t)B * 8);
  ACC* sums = reinterpret_cast<ACC*>(smem + fb + (size_t)B * 8 + kSmallValBytes);
  const XT* xrow = static_cast<const XT*>(a.X) + row * a.row_stride;
  if (FEAT_LDS) {
    for (int c = tid; c < F; c += B)
      feat[c] = c < a.n_cols ? zero_map(xrow[c], a.lgb_zero_map) : nan_value<XT>();
    __syncthreads();
  }
  const int T = a.n_trees;
  const int LW = a.leaf_width;
  const bool want_leaf = a.kind == TI_OUTPUT_LEAF;
  const bool vec = KMAX > 1 && LW > 1;         // add_leaf's third form: a vector a leaf
  const int nout = vec ? LW : 1;               // values a tree brings to the replay
  const int step = (int)(kSmallValBytes / sizeof(ACC)) / nout;   // trees a replay step
  const ACC* leaves = static_cast<const ACC*>(a.leaves);
  const int64_t last = a.sp_node_last;
  // lane k < KMAX carries output k; add_leaf leaves columns >= LW of a vector alone
  ACC acc = ACC(0);   // init_acc, column tid
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (tid == k && a.base_first) acc = (ACC)a.base[k];
  const bool col_live = tid < KMAX && (!vec || tid < LW);
  const int col = (vec && tid < LW) ? tid : 0;

  for (int t0 = 0; t0 < T; t0 += B) {
    const int n = T - t0 < B ? T - t0 : B;   // trees of this pass
    if (tid < n) {
      const int t = t0 + tid;
      const int64_t nb = a.node_base[t];
      int32_t c = a.root[t];
      while (c >= 0) {
        int64_t at = nb + c;
        at = at < last ? at : last;
        const u32x4 nd = *reinterpret_cast<const u32x4*>(a.nodes + at);   // {thr32, meta, left, right}
        const XT thr = sizeof(XT) == 4 ? (XT)__uint_as_float(nd.x) : (XT)a.thr64[at];
        const uint32_t f = nd.y & kMetaFeatMask;
        XT x;
        if (FEAT_LDS) {
          x = feat[f];
        } else {
          x = (int)f < a.n_cols ? zero_map(xrow[f], a.lgb_zero_map) : nan_value<XT>();
        }
        bool l = go_left<ZERO>(x, thr, nd.y);
        if (a.cat_words != nullptr && (nd.y & kMetaCat))
          l = (nd.y & kMetaCatXgb) ? cat_left_xgb(a.cat_words + nd.x, (double)x, nd.y)
                                   : cat_left(a.cat_words + nd.x, (double)x);
        c = l ? (int32_t)nd.z : (int32_t)nd.w;
      }
      leaf_of[tid] = ~c;
      if (!want_leaf && KMAX > 1 && !vec) grp[tid] = a.tree_group[t];
    }
    __syncthreads();
    if (want_leaf) {
      if (tid < n)
        static_cast<int32_t*>(a.out)[row * T + t0 + tid] = a.exp_leaf_ids[a.leaf_base[t0 + tid] + leaf_of[tid]];
      continue;   // a lane read its own slot: the next pass may write it
    }
    for (int s0 = 0; s0 < n; s0 += step) {
      const int m = n - s0 < step ? n - s0 : step;
      for (int e = tid; e < m * nout; e += B) {   // val[j * nout + k], the loads independent
        const int j = vec ? e / nout : e;
        const int k = vec ? e - j * nout : 0;
        const ACC* lv = leaves + a.leaf_base[t0 + s0 + j] * LW;   // add_leaf's `lv`
        val[e] = vec ? lv[(int64_t)leaf_of[s0 + j] * LW + k] : lv[leaf_of[s0 + j]];
      }
      __syncthreads();
      if (col_live) {
        if (KMAX == 1 || vec) {
          for (int j = 0; j < m; ++j) acc += val[j * nout + col];
        } else {
          for (int j = 0; j < m; ++j) acc = grp[s0 + j] == tid ? acc + val[j] : acc;
        }
      }
      __syncthreads();   // val, and after the last step leaf_of / grp, are written again
    }
  }
  if (want_leaf) return;
  if (tid < KMAX) sums[tid] = acc;
  __syncthreads();
  if (tid != 0) return;
  ACC all[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) all[k] = sums[k];
  finish_row<ACC, KMAX>(all, a, row);
}

}  // namespace ti
