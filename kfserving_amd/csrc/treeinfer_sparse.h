// treeinfer_sparse.h -- the walk of CSR rows (ti_predict_csr).
//
// A forest reads only the columns it splits on: U of them, usually a small
// part of a wide matrix.  The sparse image of a forest (built on its first CSR
// call, treeinfer.hip: ensure_sparse) is the sorted list of those columns,
// slot_of_col[F] (-1: never read) and a copy of the layout-1 nodes whose 24-bit
// feature field holds the slot.  Two regimes, one kernel:
//
//  * SEARCH = false: a workgroup owns R rows and builds the compact [U][R]
//    image of them in LDS: filled with the absent value, then overwritten from
//    the tile's contiguous run of stored entries, which the whole workgroup
//    sweeps with coalesced loads; an entry finds its row by a binary search of
//    the tile's row pointers (in LDS, log2 R steps) and its slot in
//    slot_of_col.  Entries of columns the forest never reads cost that lookup
//    and no LDS write.  The walk then is the float explicit kernel's with an
//    LDS feature image.
//  * SEARCH = true: no image.  A lane finds a node's column in its own row's
//    segment by a binary search of `indices` in global memory, the kExpIlp
//    trees of a lane searching side by side (one trip count a lane: it depends
//    on the row's length alone).  Walks the nodes that hold columns.
//
// Either way the leaves are added in tree order by add_leaf / finish_row, so
// the sums are the dense explicit kernel's bits.
#pragma once

#include "treeinfer_kernels.h"

namespace ti {

// LDS of regime A: [U][R] XT image | R + 1 tile-relative row pointers (u32).
__host__ __device__ constexpr size_t sparse_image_bytes(size_t U, size_t R, size_t xs) {
  return (U * R * xs + 15) & ~size_t(15);
}
__host__ __device__ constexpr size_t sparse_lds_bytes(size_t U, size_t R, size_t xs) {
  return sparse_image_bytes(U, R, xs) + (((R + 1) * 4 + 15) & ~size_t(15));
}

// What a slot (or a column) reads where the row stores nothing.
template <typename XT>
__device__ __forceinline__ XT sparse_absent(const KArgs& a, int32_t col) {
  return (a.sp_absent_nan != 0 || col >= a.n_cols) ? nan_value<XT>() : XT(0);
}

// Regime A, steps 1 to 4 (the header comment).  ip[j], j <= R, is row j's first
// entry relative to the tile's; rows past the batch's end are empty.
template <typename XT>
__device__ __forceinline__ void sparse_stage(XT* feat, uint32_t* ip, const KArgs& a, int64_t row0,
                                             int R, int tid) {
  const int U = a.sp_U;
  const int64_t left_rows = a.n_rows - row0;
  const int rows_here = left_rows < R ? (int)left_rows : R;
  const int64_t e0 = a.sp_indptr[row0];
  for (int u = 0; u < U; ++u) feat[u * R + tid] = sparse_absent<XT>(a, a.sp_cols[u]);
  for (int j = tid; j <= R; j += R)
    ip[j] = (uint32_t)(a.sp_indptr[row0 + (j < rows_here ? j : rows_here)] - e0);
  __syncthreads();
  const uint32_t n = ip[rows_here];
  const int32_t* idx = a.sp_indices + e0;
  const XT* val = static_cast<const XT*>(a.sp_values) + e0;
  for (uint32_t e = tid; e < n; e += R) {
    const int32_t col = idx[e];
    const XT v = val[e];
    // the last row whose first entry is at or before e: ip[R] = n > e
    int r = 0;
    for (int s = R >> 1; s > 0; s >>= 1) r = ip[r + s] <= e ? r + s : r;
    const int32_t slot = col < a.n_features ? a.sp_slot_of_col[col] : -1;
    if (slot >= 0) feat[slot * R + r] = zero_map(v, a.lgb_zero_map);
  }
  __syncthreads();
}

// Regime B: the value of column f[q] in the row's segment [s, s + len), the
// kExpIlp searches side by side.  base[q] ends at the last entry <= f[q].
template <typename XT>
__device__ __forceinline__ void sparse_find(const KArgs& a, int64_t s, uint32_t len,
                                            const uint32_t (&f)[kExpIlp], XT (&x)[kExpIlp]) {
  const int32_t* idx = a.sp_indices + s;
  const XT* val = static_cast<const XT*>(a.sp_values) + s;
  uint32_t base[kExpIlp];
#pragma unroll
  for (int q = 0; q < kExpIlp; ++q) base[q] = 0;
  for (uint32_t n = len; n > 1;) {
    const uint32_t half = n >> 1;
#pragma unroll
    for (int q = 0; q < kExpIlp; ++q)
      base[q] = (uint32_t)idx[base[q] + half] <= f[q] ? base[q] + half : base[q];
    n -= half;
  }
#pragma unroll
  for (int q = 0; q < kExpIlp; ++q) {
    x[q] = sparse_absent<XT>(a, (int32_t)f[q]);
    if (len > 0 && (uint32_t)idx[base[q]] == f[q]) x[q] = zero_map(val[base[q]], a.lgb_zero_map);
  }
}

template <typename XT, typename ACC, int KMAX, bool ZERO, bool SEARCH>
__global__ void __launch_bounds__(256) sparse_explicit_predict_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = blockDim.x;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int64_t row = row0 + tid;
  const bool live = row < a.n_rows;
  XT* feat = reinterpret_cast<XT*>(smem);
  int64_t seg = 0;
  uint32_t len = 0;
  if (SEARCH) {
    if (live) {
      seg = a.sp_indptr[row];
      len = (uint32_t)(a.sp_indptr[row + 1] - seg);
    }
  } else {
    sparse_stage<XT>(feat, reinterpret_cast<uint32_t*>(smem + sparse_image_bytes(a.sp_U, R, sizeof(XT))),
                     a, row0, R, tid);
  }
  const int T = a.n_trees;
  const bool want_leaf = a.kind == TI_OUTPUT_LEAF;
  int32_t* out_leaf = static_cast<int32_t*>(a.out);
  const ACC* leaves = static_cast<const ACC*>(a.leaves);
  const int64_t last = a.sp_node_last;   // a leaf-only last tree starts one past it

  ACC acc[KMAX];
  init_acc(acc, a);

  for (int t0 = 0; t0 < T; t0 += kExpIlp) {
    int64_t nb[kExpIlp];
    int32_t c[kExpIlp];
#pragma unroll
    for (int q = 0; q < kExpIlp; ++q) {
      const int tq = (t0 + q) < T ? (t0 + q) : (T - 1);
      nb[q] = a.node_base[tq];
      c[q] = a.root[tq];
    }
    for (;;) {
      u32x4 nd[kExpIlp];   // {thr32 bits, meta, left, right}
      XT thr[kExpIlp];
#pragma unroll
      for (int q = 0; q < kExpIlp; ++q) {
        int64_t at = nb[q] + (c[q] < 0 ? 0 : c[q]);
        at = at < last ? at : last;
        nd[q] = *reinterpret_cast<const u32x4*>(a.nodes + at);
        thr[q] = sizeof(XT) == 4 ? (XT)__uint_as_float(nd[q].x) : (XT)a.thr64[at];
      }
      XT x[kExpIlp];
      if (SEARCH) {
        uint32_t f[kExpIlp];
#pragma unroll
        for (int q = 0; q < kExpIlp; ++q) f[q] = nd[q].y & kMetaFeatMask;
        sparse_find<XT>(a, seg, len, f, x);
      } else {
#pragma unroll
        for (int q = 0; q < kExpIlp; ++q) x[q] = feat[(nd[q].y & kMetaFeatMask) * R + tid];
      }
      bool active = false;
#pragma unroll
      for (int q = 0; q < kExpIlp; ++q) {
        bool l = go_left<ZERO>(x[q], thr[q], nd[q].y);
        if (a.cat_words != nullptr && (nd[q].y & kMetaCat))   // uniform test, then rare branch
          l = (nd[q].y & kMetaCatXgb) ? cat_left_xgb(a.cat_words + nd[q].x, (double)x[q], nd[q].y)
                                      : cat_left(a.cat_words + nd[q].x, (double)x[q]);
        const int32_t next = l ? (int32_t)nd[q].z : (int32_t)nd[q].w;
        c[q] = c[q] < 0 ? c[q] : next;
        active |= c[q] >= 0;
      }
      if (__ballot(active) == 0) break;
    }
#pragma unroll
    for (int q = 0; q < kExpIlp; ++q) {
      const int t = t0 + q;
      if (t < T) {
        const int64_t lb = a.leaf_base[t];
        if (want_leaf) {
          if (live) out_leaf[row * T + t] = a.exp_leaf_ids[lb + (~c[q])];
        } else {
          add_leaf<ACC, KMAX>(acc, leaves + lb * a.leaf_width, ~c[q], a.leaf_width,
                              a.tree_group[t]);
        }
      }
    }
  }
  if (!live || want_leaf) return;
  finish_row<ACC, KMAX>(acc, a, row);
}

}  // namespace ti
