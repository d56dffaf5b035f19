// treeinfer_cheap.h — layout 10: the LDS-staged categorical heap (device code).
//
// heap_predict_kernel (treeinfer_kernels.h) for forests with categorical
// splits: the same complete-tree records, staged into LDS the same way
// (FixedSpan, stage_step), with each tree's bitsets inside its block:
//
//   [2^D - 1 HeapNode<XT>][2^D * leaf_width ACC][bitset words (u32)]
//
// A categorical node's thr field holds, as a u32 in its low word, the offset
// in u32 words from the start of its tree's block to its run
// [nwords, w0, w1, ...] (low 16 bits) and a copy of nwords (high 16 bits: a
// block is at most one stage, 64 KB, so both fit), which spares the walk the
// read of the run's first word; its meta carries kMetaCat and, for XGBoost's
// rule, kMetaCatXgb and the default child in the NaN bit.  The categorical
// nodes of a forest all use one rule (XGB template parameter); the host keeps
// a forest that mixes the two on layout 1.  tree_stride is the
// 16-byte-aligned largest block, so a stage is one contiguous copy.  The
// bitset lookup is one LDS read relative to the lane's tree pointer.
//
// Each level first asks whether any of the lane's kTilp nodes is categorical;
// only then are the categorical rules evaluated, so a level of numerical
// nodes costs what it costs in heap_stage plus that test.  The feature image
// is always in LDS (the host keeps forests too wide for it on layout 1).
#pragma once

#include "treeinfer_kernels.h"

namespace ti {

// One node as raw words: the threshold for the compare and the low word of
// the thr field for a categorical node's offset.
__device__ __forceinline__ void load_node_raw(const HeapNode<float>* p, float& thr, uint32_t& lo,
                                              uint32_t& meta) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  thr = __uint_as_float(v.x);
  lo = v.x;
  meta = v.y;
}
__device__ __forceinline__ void load_node_raw(const HeapNode<double>* p, double& thr, uint32_t& lo,
                                              uint32_t& meta) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  thr = __hiloint2double((int)v.y, (int)v.x);
  lo = v.x;
  meta = v.z;
}

// trunc(x) saturated to [0, 2^32): negative values and NaN give 0
__device__ __forceinline__ uint32_t cat_code(float x) {
  return static_cast<uint32_t>(__builtin_amdgcn_fmed3f(x, 0.0f, 4294967040.0f));
}
__device__ __forceinline__ uint32_t cat_code(double x) {
  return static_cast<uint32_t>(fmin(fmax(x, 0.0), 4294967295.0));
}

template <typename XT, typename ACC, int KMAX, bool ZERO, bool XGB, bool CHECK_NAN>
__device__ __forceinline__ void cheap_stage(const KArgs& a, const unsigned char* stage, int cnt,
                                            int t0, ACC (&acc)[KMAX], uint32_t lane_off,
                                            int64_t row, bool live) {
  using Node = HeapNode<XT>;
  const int D = a.depth;
  const int NI = (1 << D) - 1;
  const int NL = 1 << D;
  const int T = a.n_trees;
  const int64_t stride = a.tree_stride;
  const bool want_leaf = a.kind == TI_OUTPUT_LEAF;
  for (int j = 0; j < cnt; j += kTilp) {
    const Node* tp[kTilp];
#pragma unroll
    for (int q = 0; q < kTilp; ++q) {
      const int tq = (j + q) < cnt ? (j + q) : (cnt - 1);
      tp[q] = reinterpret_cast<const Node*>(stage + (int64_t)tq * stride);
    }
    uint32_t idx[kTilp];
#pragma unroll
    for (int q = 0; q < kTilp; ++q) idx[q] = 0u;
    for (int l = 0; l < D; ++l) {
      XT thr[kTilp];
      uint32_t lo[kTilp];
      uint32_t meta[kTilp];
#pragma unroll
      for (int q = 0; q < kTilp; ++q) load_node_raw(tp[q] + idx[q], thr[q], lo[q], meta[q]);
      XT x[kTilp];
#pragma unroll
      for (int q = 0; q < kTilp; ++q) x[q] = lds_at<XT>((meta[q] & kMetaFeatMask) | lane_off);
      bool left[kTilp];
      uint32_t any_meta = 0u;
#pragma unroll
      for (int q = 0; q < kTilp; ++q) {
        left[q] = go_left<ZERO, CHECK_NAN>(x[q], thr[q], meta[q]);
        any_meta |= meta[q];
      }
      if (any_meta & kMetaCat) {   // some node of this level is categorical
        // The forest's rule without a branch, the kTilp trees side by side: one
        // more LDS round trip a level (all bitset words at once), not one a
        // tree.  The category is the saturating truncation of x, so a value
        // too large for any bitset that fits a stage (>= 2^24 included) is
        // simply not a member; only the lower bound needs a compare.  A
        // numerical node reads word 0 of its block and keeps left[q].
        uint32_t v[kTilp], word[kTilp];
        bool in[kTilp];
#pragma unroll
        for (int q = 0; q < kTilp; ++q) {
          v[q] = cat_code(x[q]);
          const uint32_t off = lo[q] & 0xFFFFu, nw = lo[q] >> 16, w = v[q] >> 5;
          // XGBoost: x < 0 is invalid (-0.0 is category 0); LightGBM: x <= -1 and NaN go right
          const bool valid = XGB ? !(x[q] < XT(0)) : (x[q] > XT(-1));
          in[q] = (meta[q] & kMetaCat) && valid && w < nw;
          word[q] = reinterpret_cast<const uint32_t*>(tp[q])[in[q] ? off + 1u + w : 0u];
        }
#pragma unroll
        for (int q = 0; q < kTilp; ++q) {
          const bool member = in[q] && ((word[q] >> (v[q] & 31u)) & 1u) != 0u;
          bool cat = XGB ? !member : member;   // XGBoost: in the set -> right; invalid -> left
          if (XGB && CHECK_NAN) cat = (x[q] != x[q]) ? (int32_t)meta[q] < 0 : cat;
          left[q] = (meta[q] & kMetaCat) ? cat : left[q];
        }
      }
#pragma unroll
      for (int q = 0; q < kTilp; ++q) idx[q] = 2u * idx[q] + (left[q] ? 1u : 2u);
    }
#pragma unroll
    for (int q = 0; q < kTilp; ++q) {
      if (j + q < cnt) {
        const int leaf = (int)idx[q] - NI;
        const int t = t0 + j + q;
        if (want_leaf) {
          if (live) static_cast<int32_t*>(a.out)[row * T + t] = a.heap_leaf_ids[(int64_t)t * NL + leaf];
        } else {
          const ACC* lv = reinterpret_cast<const ACC*>(tp[q] + NI);
          add_leaf<ACC, KMAX>(acc, lv, leaf, a.leaf_width, a.tree_group[t]);
        }
      }
    }
  }
}

template <typename XT, typename ACC, int KMAX, bool ZERO, bool XGB>
__global__ void __launch_bounds__(512) cheap_predict_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Tile t = one_lane_tile(a, (uint32_t)sizeof(XT));
  const size_t feat_bytes = align16((size_t)a.n_features * t.R * sizeof(XT));
  t.flag = reinterpret_cast<volatile int*>(smem + feat_bytes);
  unsigned char* stage = smem + feat_bytes + 16;
  const bool tile_nan =
      stage_features<XT>(reinterpret_cast<XT*>(smem), t.flag, a, t.row0, t.R, t.tid);

  ACC acc[KMAX];
  init_acc(acc, a);

  // stages as in heap_predict_kernel
  const FixedSpan sp(a);
  u32x4 pf[kPf];
  stage_first(sp, pf, t.tid, t.R);
  for (int c = sp.first(); sp.more(c); c = sp.after(c)) {
    const auto st = stage_step(sp, pf, stage, c, t.tid, t.R);
    with_flag(tile_nan, [&](auto N) {
      cheap_stage<XT, ACC, KMAX, ZERO, XGB, decltype(N)::value>(a, stage, st.cnt, st.t0, acc, t.lane_off,
                                                                t.row, t.live);
    });
  }
  if (!t.live || a.kind == TI_OUTPUT_LEAF) return;
  finish_row<ACC, KMAX>(acc, a, t.row);
}

// instantiated in treeinfer_k_cat.hip, selected like every other walk
// (treeinfer_dispatch.h: Walk::CatHeapXgb / CatHeapLgb)

}  // namespace ti
