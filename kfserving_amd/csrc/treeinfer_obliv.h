// treeinfer_obliv.h — layout 12: oblivious trees (device code).
//
// In an oblivious tree (CatBoost's) every node of a level tests the same
// (feature, threshold), so a tree of depth D is D split descriptors and a
// table of 2^D leaves, and a row's leaf is  sum(bit_d << d)  of D independent
// tests.  One lane a row, as in the record layouts, over the same u16 rank-bin
// image [word][R] (rx_stage_bins):
//
//   descriptor (32 bits, layout 6's x word):  rank << 16 | bin byte offset | NaN-left
//   bit_d = rank_d < bin(feature_d)           (a NaN's bin goes by the NaN-left bit)
//
// The descriptors of a tree are the same for every lane, so they are read
// through the scalar cache from a table of their own and never enter a vector
// register or the LDS stage; the bin address is one v_or of the lane's column
// with a scalar.  A level costs one ds_read_u16 and the compare / select / or
// of its bit, and no read depends on another: the levels of a tree are issued
// eight, four or two at a time (ob_bits) and their bits OR-ed into the index,
// then the leaf is read once.  A tree's descriptors are padded to an even count
// with kObPad, whose bit is 0 on every bin.
//
// The LDS stage holds leaf tables only, 16-byte aligned, in two buffers of
// a.tree_stride bytes: stage s is committed into buffer s & 1 from the
// registers that were loaded while stage s - 1 was walked, so one barrier a
// stage is enough (a buffer is written again two stages after it was read,
// with the barrier of the stage between them).  A tree whose table is larger
// than the host's bound (plan_oblivious) is not staged: its bit 31 of rx_nint
// is set and its leaf is gathered from the image in global memory (GATHER).
// Leaves are added in tree order into the forest's accumulator type.
#pragma once

#include "treeinfer_kernels.h"

namespace ti {

// N levels of one tree from descriptor `first`, whose bits are first_bit ..
// first_bit + N - 1 of the leaf index: the N bin reads, then the N decisions.
template <int N, bool SLOW>
__device__ __forceinline__ uint32_t ob_bits(rx_cu32* desc, uint32_t first, uint32_t first_bit,
                                            uint32_t lane_off) {
  constexpr uint32_t kNan = RxBins<false>::template nan_code<false>();
  uint32_t w[N], b[N];
#pragma unroll
  for (int q = 0; q < N; ++q) w[q] = desc[first + q];
#pragma unroll
  for (int q = 0; q < N; ++q) b[q] = lds_u16((w[q] & kRxOffMask) | lane_off);
  uint32_t idx = 0u;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    bool right = (w[q] >> 16) < b[q];
    if (SLOW) right = b[q] == kNan ? (w[q] & kRxNanLeft) == 0u : right;
    idx |= right ? (1u << (first_bit + q)) : 0u;
  }
  return idx;
}

// The trees [t0, t1) of a stage whose image byte x sits at LDS address sbase + x.
template <typename ACC, int KMAX, bool SLOW, bool GATHER>
__device__ __forceinline__ void ob_stage(const KArgs& a, ACC (&acc)[KMAX], int t0, int t1,
                                         uint32_t sbase, const Tile& t) {
  rx_cu32* off = reinterpret_cast<rx_cu32*>(reinterpret_cast<uintptr_t>(a.rx_base));
  rx_cu32* dep = reinterpret_cast<rx_cu32*>(reinterpret_cast<uintptr_t>(a.rx_nint));
  rx_cu32* first = reinterpret_cast<rx_cu32*>(reinterpret_cast<uintptr_t>(a.ob_first));
  rx_cu32* goff = reinterpret_cast<rx_cu32*>(reinterpret_cast<uintptr_t>(a.ob_goff));
  rx_cu32* desc = reinterpret_cast<rx_cu32*>(reinterpret_cast<uintptr_t>(a.ob_desc));
  const int LW = a.leaf_width;
  for (int j = t0; j < t1; ++j) {
    const uint32_t dw = dep[j];
    const uint32_t d2 = ((dw & 0xFFu) + 1u) & ~1u;   // levels, pads included
    const uint32_t f0 = first[j];
    uint32_t idx = 0u, d = 0u;
    for (; d + 8u <= d2; d += 8u) idx |= ob_bits<8, SLOW>(desc, f0 + d, d, t.lane_off);
    if (d2 & 4u) {
      idx |= ob_bits<4, SLOW>(desc, f0 + d, d, t.lane_off);
      d += 4u;
    }
    if (d2 & 2u) idx |= ob_bits<2, SLOW>(desc, f0 + d, d, t.lane_off);
    if (a.kind == TI_OUTPUT_LEAF) {
      if (t.live)
        static_cast<int32_t*>(a.out)[t.row * a.n_trees + j] = a.exp_leaf_ids[a.leaf_base[j] + idx];
      continue;
    }
    ACC v[KMAX];
    if (GATHER && (dw & kObGather) != 0u) {   // uniform: the whole wave gathers this tree
      const ACC* p = reinterpret_cast<const ACC*>(a.trees + (static_cast<size_t>(goff[j]) << 4)) +
                     static_cast<size_t>(idx) * LW;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) v[k] = k < LW ? p[k] : ACC(0);
    } else {
      const uint32_t at = sbase + off[j] + idx * static_cast<uint32_t>(LW * sizeof(ACC));
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        v[k] = k < LW ? lds_at<ACC>(at + static_cast<uint32_t>(k * sizeof(ACC))) : ACC(0);
    }
    add_leaf<ACC, KMAX>(acc, v, 0, LW, a.tree_group[j]);
  }
}

// [bin image][flag][stage buffer 0][stage buffer 1]; the two buffers are the
// binning's temp area until the first commit.
template <typename XT, typename ACC, int KMAX, bool GATHER>
__global__ void __launch_bounds__(512) oblivious_predict_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int PF = 8;   // = kLxPf (host): a stage is at most PF x 16 B x R
  const Tile t = bin_tile(a, smem);
  unsigned char* stage = smem + a.stage_off;
  const uint32_t cap = static_cast<uint32_t>(a.tree_stride);
  const TreeSpan<false, CopyN> sp(a, a.trees);
  u32x4 pf[PF];
  stage_first(sp, pf, t.tid, t.R);
  // ends in a barrier: nothing reads the temp area after it
  const bool slow = rx_stage_bins<XT, false>(t.flag, a, t.row0, t.R, t.tid, stage);
  ACC acc[KMAX];
  init_acc(acc, a);
  for (int s = sp.first(); sp.more(s); s = sp.after(s)) {
    const uint32_t buf = (s & 1) ? cap : 0u;
    const auto st = sp.at(s);
    sp.template commit<PF>(pf, reinterpret_cast<u32x4*>(stage + buf), s, t.tid, t.R);
    __syncthreads();
    sp.template fetch<PF>(pf, sp.following(s), t.tid, t.R);
    with_flag(slow, [&](auto S) {
      ob_stage<ACC, KMAX, decltype(S)::value, GATHER>(a, acc, st.t0, st.t1, st.sbase + buf, t);
    });
  }
  if (!t.live || a.kind == TI_OUTPUT_LEAF) return;
  finish_row<ACC, KMAX>(acc, a, t.row);
}

// instantiated in treeinfer_k_obliv.hip (treeinfer_dispatch.h: Walk::Oblivious / ObliviousGather)

}  // namespace ti
