// treeinfer_estop.h -- LightGBM's prediction early stopping, TI_OUTPUT_EARLY_STOP
// (ABI 15): the round-checked walk.
//
// Every other walk streams all T trees past every row.  Here the forest is cut
// into rounds of R trees (ti_forest_set_early_stop); after each whole round a
// row's accumulators are tested (treeinfer.h: the rule) and a row that is far
// enough from the decision boundary adds no further tree.  The chain a row runs
// until then is TI_OUTPUT_MARGIN's: init_acc, one add_leaf a tree in tree order,
// finish_row -- so R >= T or margin = +inf give that kind's bits.
//
// Rounds-major.  A lane owns a row and a 256-lane workgroup a tile of rows; a
// launch covers a segment of consecutive rounds [es_r0, es_r1).
//
//   Image.  The layout-1 node set the CSR walk and the small-batch walk share
//   (SparsePtrs::sp_ex).  Its trees are contiguous in tree order, so round r's
//   nodes are [node_base[r R], node_base[(r + 1) R]) -- node_base is the table of
//   round ranges for every R, and R may change between calls.
//
//   LDS.  [feat: F x 256 XT, FEAT_LDS | two node buffers of es_cap nodes, each
//   u32x4 nodes then (float64 X) thr64 | three words of live counts].  A round
//   of at most es_cap nodes is copied by the whole workgroup with 16-byte loads,
//   consecutive lanes consecutive nodes, into the buffer the running round does
//   not read: its loads are issued before the lanes walk round r, stay in
//   registers (kEsPf words a lane) while they do, and are stored behind the
//   walk, so one barrier a round serves the copy and the live count.  A round
//   of more nodes is walked from global memory (clamped loads, as
//   tree_lanes_predict_kernel has them).  Either way the step is the explicit
//   kernel's -- go_left / cat_left / cat_left_xgb on {thr32, meta, left, right}
//   -- kEsIlp trees a lane at once, the adds then in tree order.
//
//   Rows.  The first segment's tile is rows [256 b, 256 b + 256) of X; a later
//   segment's is 256 entries of the survivor list the segment before wrote:
//   the row id and the K accumulators, column-major ([K][es_list_cap]).  With
//   FEAT_LDS each lane copies its row into the [f][256] image once a segment
//   (the rows of a list are scattered: no coalesced form); else it reads X.
//
//   The test.  K accumulators in registers; the top two of K is a register
//   scan.  A stopped lane runs finish_row, which writes its output row, and
//   idles: its roots read as leaves, so it issues no node load.  A wave whose
//   ballot of live lanes is empty skips the round's walk but meets the barrier;
//   a workgroup whose live count is zero leaves.
//
//   Compaction.  At the end of a segment that is not the last, a wave appends
//   its survivors to the next segment's list: ballot + mbcnt for the position
//   in the wave, one vector atomicAdd a wave on the list's count.  The next
//   launch has the worst-case grid and workgroups past the count leave at once,
//   so the host never reads a count.  The order of a list depends on the order
//   of those atomics; no result does, since each entry carries its own chain
//   and is written to its own output row.
#pragma once

#include "treeinfer_kernels.h"

namespace ti {

constexpr int kEsRows = 256;       // rows a workgroup
constexpr int kEsIlp = 4;          // trees a lane walks at once
constexpr int kEsPf = 10;          // 16-byte node words a lane holds for the next round
constexpr int kEsSegRounds = 4;    // rounds a launch (1, 2 and 8 not measured yet)
constexpr int kEsMaxCap = kEsPf * kEsRows;   // nodes a buffer holds at most

__host__ __device__ constexpr size_t estop_feat_bytes(size_t F, size_t xs) { return F * kEsRows * xs; }
__host__ __device__ constexpr size_t estop_node_bytes(size_t xs) { return xs == 8 ? 24 : 16; }
__host__ __device__ constexpr size_t estop_lds_bytes(size_t feat_bytes, size_t cap, size_t xs) {
  return feat_bytes + 2 * cap * estop_node_bytes(xs) + 16;
}
// A survivor list of `cap` entries (a multiple of 256): ids, then K columns.
__host__ __device__ constexpr size_t estop_list_bytes(size_t cap, size_t K, size_t acc_bytes) {
  return cap * 4 + K * cap * acc_bytes;
}

// The counts of the survivor lists: zero before a block's first segment (a
// kernel, not a memset: the call may be recorded into a graph).  static: the
// header is in two units, the host's and the walk's.
static __global__ void estop_clear_kernel(uint32_t* counts, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) counts[i] = 0u;
}

// The rule's test on a row's accumulators, widened to double.
template <typename ACC, int KMAX>
__device__ __forceinline__ bool estop_test(const ACC (&acc)[KMAX], int K, double m) {
  if (KMAX == 1) return 2.0 * __builtin_fabs((double)acc[0]) > m;   // false for a NaN
  double hi = (double)acc[0], lo = (double)acc[KMAX > 1 ? 1 : 0];
  bool nan = hi != hi || lo != lo;
  if (lo > hi) {
    const double t = hi;
    hi = lo;
    lo = t;
  }
#pragma unroll
  for (int k = 2; k < KMAX; ++k) {
    if (k >= K) continue;
    const double v = (double)acc[k];
    nan |= v != v;
    if (v > hi) {
      lo = hi;
      hi = v;
    } else if (v > lo) {
      lo = v;
    }
  }
  return !nan && hi - lo > m;   // a tie of the top two is 0
}

// The trees [t0, t1) of one round for this lane.  STAGED: the round's nodes are
// in LDS at `ln` (thresholds of float64 X at `lt`), node `rb` of the image first.
// `last`: the last node a load may name, of the round's in LDS or of the image;
// a lane at a leaf keeps loading a node of its tree, or that one: always a node.
template <typename XT, typename ACC, int KMAX, bool FEAT_LDS, bool ZERO, bool STAGED>
__device__ __forceinline__ void estop_round(const KArgs& a, ACC (&acc)[KMAX], int t0, int t1, bool live,
                                            const u32x4* ln, const double* lt, int64_t rb,
                                            int64_t last, const XT* feat, const XT* xrow, int tid) {
  const ACC* leaves = static_cast<const ACC*>(a.leaves);
  for (int tb = t0; tb < t1; tb += kEsIlp) {
    int64_t nb[kEsIlp];
    int32_t c[kEsIlp];
#pragma unroll
    for (int q = 0; q < kEsIlp; ++q) {
      const int tq = (tb + q) < t1 ? (tb + q) : (t1 - 1);
      nb[q] = a.node_base[tq] - (STAGED ? rb : 0);
      c[q] = live ? a.root[tq] : ~0;   // an idle lane is at a leaf already
    }
    for (;;) {
      u32x4 nd[kEsIlp];
      XT thr[kEsIlp];
#pragma unroll
      for (int q = 0; q < kEsIlp; ++q) {
        int64_t at = nb[q] + (c[q] < 0 ? 0 : c[q]);
        at = at < last ? at : last;
        nd[q] = STAGED ? ln[at] : *reinterpret_cast<const u32x4*>(a.nodes + at);
        thr[q] = sizeof(XT) == 4 ? (XT)__uint_as_float(nd[q].x) : (XT)(STAGED ? lt[at] : a.thr64[at]);
      }
      bool active = false;
#pragma unroll
      for (int q = 0; q < kEsIlp; ++q) {
        const uint32_t f = nd[q].y & kMetaFeatMask;
        XT x;
        if (FEAT_LDS) {
          x = feat[f * kEsRows + tid];
        } else {
          x = (int)f < a.n_cols ? zero_map(xrow[f], a.lgb_zero_map) : nan_value<XT>();
        }
        bool l = go_left<ZERO>(x, thr[q], nd[q].y);
        if (a.cat_words != nullptr && (nd[q].y & kMetaCat))
          l = (nd[q].y & kMetaCatXgb) ? cat_left_xgb(a.cat_words + nd[q].x, (double)x, nd[q].y)
                                      : cat_left(a.cat_words + nd[q].x, (double)x);
        const int32_t next = l ? (int32_t)nd[q].z : (int32_t)nd[q].w;
        c[q] = c[q] < 0 ? c[q] : next;
        active |= c[q] >= 0;
      }
      if (__ballot(active) == 0) break;
    }
    if (!live) continue;
#pragma unroll
    for (int q = 0; q < kEsIlp; ++q) {
      const int t = tb + q;
      if (t < t1)
        add_leaf<ACC, KMAX>(acc, leaves + a.leaf_base[t] * a.leaf_width, ~c[q], a.leaf_width,
                            a.tree_group[t]);
    }
  }
}

template <typename XT, typename ACC, int KMAX, bool FEAT_LDS, bool ZERO>
__global__ void __launch_bounds__(kEsRows) estop_walk_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool X64 = sizeof(XT) == 8;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int K = a.n_groups;
  const int64_t LC = a.es_list_cap;

  // this lane's row and where its chain stands
  int64_t row;
  bool live;
  ACC acc[KMAX];
  if (a.es_in == nullptr) {
    row = (int64_t)blockIdx.x * kEsRows + tid;
    live = row < a.n_rows;
    if (!live) row = a.n_rows - 1;
    init_acc(acc, a);
  } else {
    const int64_t n = *a.es_in_n;
    const int64_t at0 = (int64_t)blockIdx.x * kEsRows;
    if (at0 >= n) return;   // uniform: a workgroup past the list
    live = at0 + tid < n;
    const int64_t at = live ? at0 + tid : n - 1;
    row = static_cast<const int32_t*>(a.es_in)[at];
    const ACC* col = reinterpret_cast<const ACC*>(static_cast<const unsigned char*>(a.es_in) + LC * 4);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = k < K ? col[k * LC + at] : ACC(0);
  }

  const int F = a.n_features;
  const size_t fb = FEAT_LDS ? estop_feat_bytes(F, sizeof(XT)) : 0;
  const int cap = a.es_cap;
  XT* feat = reinterpret_cast<XT*>(smem);
  unsigned char* bufs = smem + fb;
  const size_t buf_bytes = (size_t)cap * estop_node_bytes(sizeof(XT));
  volatile int* alive = reinterpret_cast<volatile int*>(bufs + 2 * buf_bytes);   // [3]
  const XT* xrow = static_cast<const XT*>(a.X) + row * a.row_stride;
  if (FEAT_LDS) {
    for (int c = 0; c < F; ++c)
      feat[c * kEsRows + tid] = c < a.n_cols ? zero_map(xrow[c], a.lgb_zero_map) : nan_value<XT>();
  }

  const int T = a.n_trees;
  const int R = a.es_round;
  const int64_t n_nodes = a.sp_node_last + 1;
  // round r: its trees end at t1, its nodes are [*b, *b + n)
  auto round_nodes = [&](int r, int64_t* b) -> int64_t {
    const int t0 = r * R;
    const int t1 = T - t0 < R ? T : t0 + R;
    *b = a.node_base[t0];
    return (t1 < T ? a.node_base[t1] : n_nodes) - *b;
  };
  // the copy of a round, in two halves: loads into registers, stores to LDS
  u32x4 pf[kEsPf];
  uint2 pt[X64 ? kEsPf : 1];
  auto load_round = [&](int64_t b, int64_t n) {
#pragma unroll
    for (int i = 0; i < kEsPf; ++i) {
      const int e = i * kEsRows + tid;
      if (e < n) {
        pf[i] = *reinterpret_cast<const u32x4*>(a.nodes + b + e);
        if (X64) pt[i] = *reinterpret_cast<const uint2*>(a.thr64 + b + e);
      }
    }
  };
  auto store_round = [&](unsigned char* buf, int64_t n) {
    u32x4* ln = reinterpret_cast<u32x4*>(buf);
    uint2* lt = reinterpret_cast<uint2*>(buf + (size_t)cap * 16);
#pragma unroll
    for (int i = 0; i < kEsPf; ++i) {
      const int e = i * kEsRows + tid;
      if (e < n) {
        ln[e] = pf[i];
        if (X64) lt[e] = pt[i];
      }
    }
  };

  int64_t rb = 0, rn = round_nodes(a.es_r0, &rb);
  if (rn <= cap) {
    load_round(rb, rn);
    store_round(bufs, rn);
  }
  if (tid < 3) alive[tid] = 0;
  __syncthreads();

  int slot = 0;   // the live count's word, one of three in rotation
  for (int r = a.es_r0; r < a.es_r1; ++r, slot = slot == 2 ? 0 : slot + 1) {
    const bool more = r + 1 < a.es_r1;
    int64_t nxb = 0, nxn = 0;
    if (more) {
      nxn = round_nodes(r + 1, &nxb);
      if (nxn <= cap) load_round(nxb, nxn);   // in flight while this round is walked
    }
    const int t0 = r * R;
    const int t1 = T - t0 < R ? T : t0 + R;
    if (__ballot(live) != 0) {
      unsigned char* buf = bufs + (size_t)((r - a.es_r0) & 1) * buf_bytes;
      const u32x4* ln = reinterpret_cast<const u32x4*>(buf);
      const double* lt = reinterpret_cast<const double*>(buf + (size_t)cap * 16);
      if (rn > 0 && rn <= cap)
        estop_round<XT, ACC, KMAX, FEAT_LDS, ZERO, true>(a, acc, t0, t1, live, ln, lt, rb, rn - 1, feat, xrow,
                                                         tid);
      else   // too many nodes for a buffer, or none at all: trees of one leaf
        estop_round<XT, ACC, KMAX, FEAT_LDS, ZERO, false>(a, acc, t0, t1, live, ln, lt, rb, a.sp_node_last,
                                                          feat, xrow, tid);
      // a whole round of R trees is tested; a shorter tail is not
      if (live && t1 - t0 == R && estop_test<ACC, KMAX>(acc, K, a.es_margin)) {
        finish_row<ACC, KMAX>(acc, a, row);
        live = false;
      }
    }
    const uint64_t lv = __ballot(live);
    if (lane == 0 && lv != 0) atomicAdd(const_cast<int*>(alive + slot), __popcll(lv));
    // the other buffer: round r - 1 read it, and everybody has passed that round's barrier
    if (more && nxn <= cap) store_round(bufs + (size_t)((r + 1 - a.es_r0) & 1) * buf_bytes, nxn);
    __syncthreads();
    if (alive[slot] == 0) return;   // uniform: every row of the tile has stopped
    // round r - 1's word, which everybody read before this barrier; round r + 2 counts in it
    if (tid == 0) alive[slot == 0 ? 2 : slot - 1] = 0;
    rb = nxb;
    rn = nxn;
  }

  if (a.es_last) {
    if (live) finish_row<ACC, KMAX>(acc, a, row);
    return;
  }
  // survivors to the next segment's list
  const uint64_t lv = __ballot(live);
  if (lv == 0) return;
  uint32_t base = 0;
  if (lane == __ffsll((unsigned long long)lv) - 1) base = atomicAdd(a.es_out_n, (uint32_t)__popcll(lv));
  base = __shfl(base, __ffsll((unsigned long long)lv) - 1);
  if (!live) return;
  const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(lv >> 32),
                                                       __builtin_amdgcn_mbcnt_lo((uint32_t)lv, 0u));
  static_cast<int32_t*>(a.es_out)[at] = (int32_t)row;
  ACC* col = reinterpret_cast<ACC*>(static_cast<unsigned char*>(a.es_out) + LC * 4);
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) col[k * LC + at] = acc[k];
}

}  // namespace ti
