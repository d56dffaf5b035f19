// treeinfer_crec.h — layout 11: LDS-staged records for forests with
// categorical splits (device code).
//
// Layout 7 (lexplicit_predict_kernel) with two additions.  The u16 bin image
// holds, for a categorical feature, the category code of the value instead of
// a rank (cat_bin, treeinfer_kernels.h): trunc(x) below the feature's limit
// L_f, and L_f itself for every value that goes where non-members go.  And a
// tree's block is its records followed by the bitset runs of its categorical
// nodes, so the runs move through the stage pipeline with the tree:
//
//   [nint internal records][leaf records][run][run]...      (8-byte slots)
//
// A categorical internal record is
//   x = run byte offset in the block << 16 | bin byte offset | kCrCat | NaN-left
//   y = right child byte offset << 16 | left child byte offset
// and its run is the node's bitset padded with zero words to W_f + 1 words,
// W_f the longest bitset on the feature (L_f = 32 W_f).  Every code 0 .. L_f
// then has its bit inside the run, so membership is one LDS read at
//   block + run offset + (code >> 5) * 4
// -- an address made of the record and the bin alone, no length read first --
// and code L_f reads the zero word: not a member.  One predicate decides both
// rules (XGB template parameter, one rule a forest):
//   LightGBM: left = member          XGBoost: left = NaN ? NaN-left : !member
// A step reads the bin and decides numerically as layout 7 does, then asks
// once per wave whether any of the lane's ILP records is categorical; only
// then are the ILP membership words read, as one batch, and the categorical
// records' children selected from them.  No branch per tree.
//
// The unit that instantiates this header is compiled without packed float32
// arithmetic (__graft_entry__.py, UNIT_FLAGS; DESIGN.md 3.3.1 says why).
#pragma once

#include "treeinfer_kernels.h"

namespace ti {

// rx_bin_addr with the categorical flag cleared as well
__device__ __forceinline__ uint32_t cr_bin_addr(uint32_t x, bool in, uint32_t lane_off) {
  uint32_t t = (x & kCrOffMask) | lane_off;
  asm("" : "+v"(t));
  return in ? t : lane_off;
}

template <typename ACC, int KMAX, bool ZERO, bool SLOW, bool VIS, int ILP, bool XGB>
__device__ __forceinline__ void cr_stage(const KArgs& a, ACC (&acc)[KMAX], int t0, int t1,
                                         uint32_t sbase, const Tile& t) {
  constexpr uint32_t kNan = RxBins<false>::template nan_code<ZERO>();
  rx_cu32* rx_base = reinterpret_cast<rx_cu32*>(reinterpret_cast<uintptr_t>(a.rx_base));
  rx_cu32* rx_nint = reinterpret_cast<rx_cu32*>(reinterpret_cast<uintptr_t>(a.rx_nint));
  for (int j = t0; j < t1; j += ILP) {
    uint32_t base[ILP], ni8[ILP], at[ILP];   // block base (LDS), internal bytes, lane's byte
    rx_u2_t rec[ILP];
#pragma unroll
    for (int q = 0; q < ILP; ++q) {
      const int tq = (j + q) < t1 ? (j + q) : (t1 - 1);
      base[q] = sbase + (rx_base[tq] << 3);
      ni8[q] = rx_nint[tq] << 3;
      at[q] = 0u;
      rec[q] = lx_rec(base[q]);
    }
    for (;;) {
      bool in[ILP], cat[ILP];
      uint32_t b[ILP], nx[ILP];
      bool any = false, any_cat = false;
#pragma unroll
      for (int q = 0; q < ILP; ++q) {
        in[q] = at[q] < ni8[q];
        any |= in[q];
        cat[q] = in[q] && (rec[q].x & kCrCat) != 0u;   // a leaf record's x holds value bits
        any_cat |= cat[q];
        b[q] = lds_u16(cr_bin_addr(rec[q].x, in[q], t.lane_off));
      }
#pragma unroll
      for (int q = 0; q < ILP; ++q) nx[q] = rx_next<ZERO, SLOW>(rec[q].x, rec[q].y, (uint16_t)b[q]);
      if (__ballot(any_cat) != 0) {   // some lane of the wave stands on a categorical record
        uint32_t w[ILP];
#pragma unroll
        for (int q = 0; q < ILP; ++q) {
          // a NaN (XGBoost's rule) has no bit and reads word 0: in slow tiles,
          // and in any tile the lanes past the last row, binned from nothing
          const uint32_t code = (XGB && b[q] == kNan) ? 0u : b[q];
          const uint32_t run = base[q] + (rec[q].x >> 16) + ((code >> 5) << 2);
          w[q] = lds_u32(cat[q] ? run : base[q]);   // others: the block's first word, a broadcast
        }
#pragma unroll
        for (int q = 0; q < ILP; ++q) {
          const bool member = ((w[q] >> (b[q] & 31u)) & 1u) != 0u;
          bool right = XGB ? member : !member;
          if (XGB && SLOW) right = b[q] == kNan ? (rec[q].x & kRxNanLeft) == 0u : right;
          const uint32_t child = right ? (rec[q].y >> 16) : (rec[q].y & 0xFFFFu);
          nx[q] = cat[q] ? child : nx[q];
        }
      }
#pragma unroll
      for (int q = 0; q < ILP; ++q) {
        at[q] = in[q] ? nx[q] : at[q];
        rec[q] = lx_rec(base[q] + at[q]);
      }
      if (__ballot(any) == 0) break;
    }
#pragma unroll
    for (int q = 0; q < ILP; ++q)
      if (j + q < t1)
        rx_leaves<ACC, KMAX>(a, acc, j + q, at[q] >> 3, ni8[q] >> 3, rec[q].x, rec[q].y, t.row,
                             t.live, VIS);
  }
}

// lexplicit_predict_kernel's frame: the first stage's loads in flight while the
// tile is binned (categorical columns coded by the forest's rule), then a
// stage handed over per pass and walked by cr_stage.
template <typename XT, typename ACC, int KMAX, bool ZERO, int ILP, bool XGB>
__global__ void __launch_bounds__(512) crexplicit_predict_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int PF = 8;   // = kLxPf (host): a stage is at most PF x 16 B x R
  const Tile t = bin_tile(a, smem);
  unsigned char* stage = smem + a.stage_off;
  const TreeSpan<true, CopyN> sp(a, a.rx_recs);
  u32x4 pf[PF];
  stage_first(sp, pf, t.tid, t.R);
  const bool slow = rx_stage_bins<XT, ZERO, false, false, XGB ? 2 : 1>(t.flag, a, t.row0, t.R, t.tid, stage);
  const bool vis = a.leaf_width == 1 && a.kind != TI_OUTPUT_LEAF;
  ACC acc[KMAX];
  init_acc(acc, a);
  for (int c = sp.first(); sp.more(c); c = sp.after(c)) {
    const auto st = stage_step(sp, pf, stage, c, t.tid, t.R);
    with_flags(slow, vis, [&](auto S, auto V) {
      cr_stage<ACC, KMAX, ZERO, decltype(S)::value, decltype(V)::value, ILP, XGB>(a, acc, st.t0, st.t1,
                                                                                  st.sbase, t);
    });
  }
  if (!t.live || a.kind == TI_OUTPUT_LEAF) return;
  finish_row<ACC, KMAX>(acc, a, t.row);
}

// instantiated in treeinfer_k_crec.hip (treeinfer_dispatch.h: Walk::CatRecordXgb / CatRecordLgb)

}  // namespace ti
