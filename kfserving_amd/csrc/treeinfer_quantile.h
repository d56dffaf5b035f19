// treeinfer_quantile.h — weighted quantiles across a row's per-tree predictions,
// TI_OUTPUT_TREE_QUANTILE (ABI 11; sklearn's AdaBoostRegressor.predict, and
// per-row quantiles of an averaging forest): the host tables (keep_quantile_source,
// ensure_quantile) and the second of launch_quantile's two stream-ordered
// passes (treeinfer.hip).  Included by treeinfer.hip alone.
//
// Pass 1 is the forest's own walk with TI_OUTPUT_LEAF into a [rows, T] int32
// scratch.  Pass 2, here, reads no X.  For a row it gathers the T leaf values,
// orders the trees by (value, tree index), forms the cumulative weight in that
// order -- one float64 add a position, never a tree of adds: a cumulative
// weight within rounding of a threshold must land where numpy's cumsum puts
// it -- and answers every level q with the value at the first position whose
// cumulative weight reaches fl(q * total).
//
// Tables (per replica, uploaded on the first call: ensure_quantile):
//   leaf_base [T + 1]   first value of each tree; tree t's value of the leaf
//                       whose library id is i sits at leaf_base[t] + i
//                       (treeinfer_approx.h's addressing: ids non-negative and
//                       distinct within a tree, neither dense nor node indexes)
//   values    [sum over trees of (largest leaf id + 1)]  float64
//   weights   [T]       float64 (1.0 each when the descriptor gave none)
//
// Sort keys.  A key is {the value's float64 bits mapped to an unsigned integer
// of the same order, the tree index}: -0.0 maps to +0.0's key and every NaN to
// one key above +inf, so equal values tie and fall to the tree index, as the
// rule says.  Padding up to the network's power of two is the all-ones key,
// above every real one.  A key does not carry its value back: the answer is
// re-read from the table through the winning tree's leaf id, so it is the
// table's element bit for bit, NaN payloads and the sign of zero included.
//
// Two kernels, by the network's size N = the power of two >= max(T, 64):
//
// N <= 512 (tree_quantile_reg_kernel<NK>, NK = N / 64 keys a lane).  A wave
// owns a row while it sorts.  The lanes read the row's ids coalesced along T
// (lane l, key k reads tree k * 64 + l: a bitonic network orders whatever it
// is given), and element lane * NK + k of the network lives in register k of
// the lane.  Compare distances below NK are exchanges between a lane's own
// registers; distances of NK and more pair lane l with lane l ^ J, J = 1..32,
// and move the three key words by DPP quad_perm (J = 1, 2), ds_swizzle in bit
// mode (J = 4, 8, 16) and ds_bpermute (J = 32): the crossbar, no LDS memory.
// AdaBoost's default T = 50 is NK = 1, 21 exchange steps, all cross-lane.
// The cumulative sum is a chain of T dependent adds, so one lane a row is all
// it can use: a wave sorts kQRowsPerWave rows one after the other, leaves each
// row's order in LDS as 16-bit tree indexes (row pitch N + 2: an odd number of
// dwords, so the lanes of the scan fall in distinct banks), and then lane r of
// the wave scans row r -- kQRowsPerWave chains in flight a wave instead of one.
// The total is needed before the thresholds: the chain runs twice (keeping the
// cdf would cost 8 bytes a position where the order costs 2).  Four waves, 64
// rows a workgroup; LDS is 8 T bytes of weights and 64 (N + 2) 2-byte indexes:
// 8.6 KiB at N = 64, 68 KiB at N = 512.
//
// N = 1024 .. 4096 (tree_quantile_lds_kernel).  192 key registers a lane would
// be needed at N = 4096, so the keys live in LDS, 12 bytes each, and a wave
// runs the same network over them.  A wave's keys are its own slice of LDS, so
// a step ends in a wave-local synchronisation (a wavefront fence and
// s_wave_barrier: LDS serves one wave's instructions in order), never in a
// workgroup barrier, and the waves of a workgroup do not wait for each other.  48 KiB of
// keys a workgroup whatever N is: four waves (rows) at N = 1024, two at 2048,
// one at 4096, three workgroups a CU.  After the sort the key words are
// overwritten with the sorted weights, and lane 0 scans them: consecutive
// float64 from LDS, broadcast reads.  The scan is a quarter of the sort's time
// there (2 T dependent adds against 78 steps of N / 128 exchanges a lane), so
// the transposition of the register kernel is not repeated.
//
// Neither kernel uses atomics or reads what it wrote to global memory: two
// calls give the same bits.  Float64 values and weights for every forest:
// float32 leaf values widen exactly and round back exactly.
#pragma once

#include "treeinfer_forest.h"

namespace ti {

constexpr int kQuantileMaxTrees = 4096;   // the cap: N = 4096 keys are 48 KiB of LDS a row
constexpr int kQuantileMaxLevels = 8;
constexpr int kQRegMaxN = 512;            // largest network held in registers (8 keys a lane)
constexpr int kQWaves = 4;                // register kernel: waves a workgroup
constexpr int kQRowsPerWave = 16;         //   rows a wave sorts, then scans side by side
constexpr int kQRegRows = kQWaves * kQRowsPerWave;
constexpr int kQLdsRowsPerWave = 4;       // LDS kernel: rows a wave handles, one after the other
constexpr uint32_t kQLdsKeyBytes = 48 * 1024;   // LDS kernel: key bytes a workgroup

struct QuantileArgs {
  const int32_t* leaf_ids;    // [n_rows][T] pass 1's output for the rows of this launch
  const int64_t* leaf_base;   // [T + 1]
  const double* values;
  const double* weights;      // [T]
  double q[kQuantileMaxLevels];
  int32_t n_q;
  int32_t n_trees;
  int64_t n_rows;
  void* out;                  // [n_rows][n_q], float32 or float64
  int32_t out_f32;
  int32_t n_pad;              // N (LDS kernel)
};

// The value of tree t for a row, and its sort key.  A tree index past the
// forest, or an id outside its tree's values (no sort and no walk reports
// one), reads as NaN, not past the tables.
__device__ __forceinline__ double quantile_value(const QuantileArgs& a, const int32_t* ids, int t) {
  if ((uint32_t)t >= (uint32_t)a.n_trees) return __longlong_as_double(0x7ff8000000000000LL);
  const int64_t lb = a.leaf_base[t];
  const int64_t id = ids[t];
  if ((uint64_t)id >= (uint64_t)(a.leaf_base[t + 1] - lb)) return __longlong_as_double(0x7ff8000000000000LL);
  return a.values[lb + id];
}

__device__ __forceinline__ uint64_t quantile_key(double v) {
  if (v != v) return 0xfffffffffffffffeull;          // every NaN: above +inf, below the padding
  if (v == 0.0) return 0x8000000000000000ull;        // -0.0 ties with +0.0
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ void quantile_store(const QuantileArgs& a, int64_t row, int q, double v) {
  const int64_t e = row * a.n_q + q;
  if (a.out_f32) static_cast<float*>(a.out)[e] = (float)v;
  else static_cast<double*>(a.out)[e] = v;
}

// One word from lane (l ^ J) of the wave.
template <int J>
__device__ __forceinline__ uint32_t quantile_xlane(uint32_t v) {
  if constexpr (J == 1) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
  } else if constexpr (J == 2) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
  } else if constexpr (J < 32) {
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (J << 10) | 0x1f);    // bit mode: and 0x1f, xor J
  } else {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((threadIdx.x & 63) ^ 32) << 2), (int)v);
  }
}

struct QKey {
  uint64_t key;
  uint32_t tree;
};
__device__ __forceinline__ bool quantile_gt(const QKey& a, const QKey& b) {
  return a.key > b.key || (a.key == b.key && a.tree > b.tree);
}

// One step of the network at distance J lanes: every register meets the same
// register of lane l ^ J.  KK: the size of the bitonic runs being merged, in
// elements; an element's direction is bit KK of its index lane * NK + k.
template <int NK, int KK, int J>
__device__ __forceinline__ void quantile_cross_step(QKey (&e)[NK], int lane) {
  const bool lower = (lane & J) == 0;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    QKey o;
    o.key = ((uint64_t)quantile_xlane<J>((uint32_t)(e[k].key >> 32)) << 32) |
            quantile_xlane<J>((uint32_t)e[k].key);
    o.tree = quantile_xlane<J>(e[k].tree);
    const bool up = ((lane * NK + k) & KK) == 0;
    // the lower element keeps the smaller key of an ascending pair
    const bool take = (lower == up) ? quantile_gt(e[k], o) : quantile_gt(o, e[k]);
    if (take) e[k] = o;
  }
}

template <int NK, int KK, int J>
__device__ __forceinline__ void quantile_local_step(QKey (&e)[NK], int lane) {
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (k & J) continue;
    const bool up = ((lane * NK + k) & KK) == 0;
    if (quantile_gt(e[k], e[k | J]) == up) {
      const QKey t = e[k];
      e[k] = e[k | J];
      e[k | J] = t;
    }
  }
}

template <int NK, int KK, int J>
__device__ __forceinline__ void quantile_merge(QKey (&e)[NK], int lane) {
  if constexpr (J >= NK) quantile_cross_step<NK, KK, J / NK>(e, lane);
  else quantile_local_step<NK, KK, J>(e, lane);
  if constexpr (J > 1) quantile_merge<NK, KK, J / 2>(e, lane);
}

template <int NK, int KK>
__device__ __forceinline__ void quantile_sort(QKey (&e)[NK], int lane) {
  if constexpr (KK > 2) quantile_sort<NK, KK / 2>(e, lane);
  quantile_merge<NK, KK, KK / 2>(e, lane);
}

// The two chains of one row over its sorted weights: the total, then the first
// position at or above each threshold.  weight(p) is position p's weight;
// first[q] stays 0 where no position qualifies (a NaN threshold: 0 * inf), as
// numpy's argmax of an all-false mask does.
template <typename W>
__device__ __forceinline__ void quantile_scan(const QuantileArgs& a, int T, W weight,
                                              int (&first)[kQuantileMaxLevels]) {
  double c = 0.0;
  for (int p = 0; p < T; ++p) c = c + weight(p);
  double thr[kQuantileMaxLevels];
  uint32_t open = 0;
#pragma unroll
  for (int q = 0; q < kQuantileMaxLevels; ++q) {
    thr[q] = a.q[q] * c;
    first[q] = 0;
    if (q < a.n_q) open |= 1u << q;
  }
  c = 0.0;
  for (int p = 0; p < T && open; ++p) {
    c = c + weight(p);
#pragma unroll
    for (int q = 0; q < kQuantileMaxLevels; ++q)
      if ((open >> q & 1u) && c >= thr[q]) {
        first[q] = p;
        open &= ~(1u << q);
      }
  }
}

template <int NK>
__global__ void __launch_bounds__(kQWaves * 64) tree_quantile_reg_kernel(const QuantileArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int N = NK * 64;
  constexpr int P = N + 2;   // uint16 entries between two rows' orders
  const int T = a.n_trees;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  double* wl = reinterpret_cast<double*>(smem);                               // [T]
  uint16_t* ord = reinterpret_cast<uint16_t*>(smem + (((size_t)T * 8 + 15) & ~size_t(15)));   // [kQRegRows][P]
  for (int t = tid; t < T; t += kQWaves * 64) wl[t] = a.weights[t];
  const int64_t row0 = (int64_t)blockIdx.x * kQRegRows + wave * kQRowsPerWave;

  for (int r = 0; r < kQRowsPerWave; ++r) {
    const int64_t row = row0 + r;
    if (row >= a.n_rows) break;   // the wave's own rows: uniform over its lanes
    const int32_t* ids = a.leaf_ids + row * (int64_t)T;
    QKey e[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int t = k * 64 + lane;
      e[k].key = ~0ull;
      e[k].tree = 0xffffffffu;
      if (t < T) {
        e[k].key = quantile_key(quantile_value(a, ids, t));
        e[k].tree = (uint32_t)t;
      }
    }
    quantile_sort<NK, N>(e, lane);
    uint16_t* o = ord + (size_t)(wave * kQRowsPerWave + r) * P + lane * NK;
#pragma unroll
    for (int k = 0; k < NK; ++k) o[k] = (uint16_t)e[k].tree;
  }
  __syncthreads();   // the weights and every wave's orders are in LDS

  const int64_t row = row0 + lane;
  if (lane >= kQRowsPerWave || row >= a.n_rows) return;
  const uint16_t* o = ord + (size_t)(wave * kQRowsPerWave + lane) * P;
  int first[kQuantileMaxLevels];
  quantile_scan(a, T, [&](int p) { return wl[o[p]]; }, first);
  const int32_t* ids = a.leaf_ids + row * (int64_t)T;
#pragma unroll
  for (int q = 0; q < kQuantileMaxLevels; ++q)   // unrolled: first[] stays in registers
    if (q < a.n_q) quantile_store(a, row, q, quantile_value(a, ids, o[first[q]]));
}

// What a wave wrote to its LDS slice is read by other lanes of the same wave
// next: the compiler may not move LDS accesses across this point, and the
// hardware serves a wave's LDS instructions in order.
__device__ __forceinline__ void quantile_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// blockDim.x = 64 * waves, waves * n_pad * 12 = kQLdsKeyBytes of dynamic LDS.
// The waves share nothing: each sorts its own rows in its own slice.
__global__ void __launch_bounds__(256) tree_quantile_lds_kernel(const QuantileArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int N = a.n_pad;
  const int T = a.n_trees;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  uint64_t* key = reinterpret_cast<uint64_t*>(smem) + (size_t)wave * N;                   // [N]
  uint32_t* tree = reinterpret_cast<uint32_t*>(smem + (size_t)waves * N * 8) + (size_t)wave * N;   // [N]
  double* ws = reinterpret_cast<double*>(key);   // the sorted weights, once the keys are spent

  for (int r = 0; r < kQLdsRowsPerWave; ++r) {
    const int64_t row = ((int64_t)blockIdx.x * waves + wave) * kQLdsRowsPerWave + r;
    if (row >= a.n_rows) break;   // the wave's own rows: uniform over its lanes
    const int32_t* ids = a.leaf_ids + row * (int64_t)T;
    for (int t = lane; t < N; t += 64) {
      const bool real = t < T;
      key[t] = real ? quantile_key(quantile_value(a, ids, t)) : ~0ull;
      tree[t] = real ? (uint32_t)t : 0xffffffffu;
    }
    quantile_wave_sync();
    for (int kk = 2; kk <= N; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int p = lane; p < (N >> 1); p += 64) {
          const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
          const int l = i | j;
          const QKey x{key[i], tree[i]}, y{key[l], tree[l]};
          if (quantile_gt(x, y) == ((i & kk) == 0)) {
            key[i] = y.key;
            tree[i] = y.tree;
            key[l] = x.key;
            tree[l] = x.tree;
          }
        }
        quantile_wave_sync();
      }
    }
    for (int p = lane; p < T; p += 64)   // position p's own slot; the T real keys sort first
      ws[p] = tree[p] < (uint32_t)T ? a.weights[tree[p]] : 0.0;
    quantile_wave_sync();
    if (lane == 0) {
      int first[kQuantileMaxLevels];
      quantile_scan(a, T, [&](int p) { return ws[p]; }, first);
#pragma unroll
      for (int q = 0; q < kQuantileMaxLevels; ++q)
        if (q < a.n_q) quantile_store(a, row, q, quantile_value(a, ids, (int)tree[first[q]]));
    }
    quantile_wave_sync();   // the next row's keys overwrite these
  }
}

}  // namespace ti

namespace {

void free_quantile(DeviceForest& d) {
  d.quant_mem.release();
  static_cast<QuantilePtrs&>(d) = QuantilePtrs();
}

// At create: whether the kind is possible, and the host tables ensure_quantile
// uploads on first use (they are a fraction of the descriptor: one float64 a
// leaf id, two a tree).
void keep_quantile_source(const ti_forest_desc* d, ti_forest* f) {
  auto refuse = [&](const std::string& why) { f->quant_refused = "TI_OUTPUT_TREE_QUANTILE " + why; };
  if (d->leaf_width != 1 || d->n_groups != 1)
    return refuse("needs one scalar prediction a tree (leaf_width == 1 and n_groups == 1)");
  if (d->lin_offset) return refuse("of a forest with linear leaves (a leaf has no one value to order)");
  if (d->n_trees > ti::kQuantileMaxTrees)
    return refuse("serves at most " + std::to_string(ti::kQuantileMaxTrees) + " trees, the forest has " +
                  std::to_string(d->n_trees));
  auto tab = std::make_unique<ti_forest::QuantileTables>();
  const int T = d->n_trees;
  tab->leaf_base.assign(T + 1, 0);
  for (int t = 0; t < T; ++t) {
    int64_t top = -1;
    bool negative = false;
    for (int64_t g = d->tree_offset[t]; g < d->tree_offset[t + 1]; ++g)
      if (d->feature[g] < 0) {
        negative |= d->leaf_id[g] < 0;
        top = std::max<int64_t>(top, d->leaf_id[g]);
      }
    // distinct ids: every slot of the tree's range is written at most once
    const size_t base = tab->values.size();
    std::vector<char> seen(negative || top < 0 ? 0 : static_cast<size_t>(top) + 1, 0);
    bool distinct = !negative;
    if (distinct) {
      tab->values.resize(base + seen.size(), std::numeric_limits<double>::quiet_NaN());
      for (int64_t g = d->tree_offset[t]; g < d->tree_offset[t + 1] && distinct; ++g)
        if (d->feature[g] < 0) {
          if (seen[d->leaf_id[g]]) distinct = false;
          seen[d->leaf_id[g]] = 1;
          tab->values[base + d->leaf_id[g]] = d->leaf_value[g];
        }
    }
    if (!distinct)
      return refuse("finds a tree's value by its leaf id: tree " + std::to_string(t) +
                    " has leaf ids that are negative or not distinct");
    tab->leaf_base[t + 1] = static_cast<int64_t>(tab->values.size());
  }
  tab->weights.assign(T, 1.0);
  if (d->tree_weight) tab->weights.assign(d->tree_weight, d->tree_weight + T);
  f->quant_tab = std::move(tab);
}

// First TI_OUTPUT_TREE_QUANTILE call of a handle: upload the tables to every
// replica, under the forest's lock (ensure_approx's lifecycle: predict-only
// serving pays nothing on the device, the bytes count in device_bytes, a failed
// upload frees every replica's tables and restores the counts).
int ensure_quantile(ti_forest* f) {
  if (f->quant_ready.load(std::memory_order_acquire)) return TI_OK;
  std::lock_guard<std::mutex> lk(f->shap_mu);
  if (f->quant_ready.load(std::memory_order_relaxed)) return TI_OK;
  const ti_forest::QuantileTables& tab = *f->quant_tab;
  int dev0 = 0, rc = TI_OK;
  TI_HIP(hipGetDevice(&dev0));
  std::vector<int64_t> bytes0;
  for (auto& dp : f->devs) bytes0.push_back(dp->bytes);
  for (auto& dp : f->devs) {
    DeviceForest& d = *dp;
    if ((rc = fail_hip(hipSetDevice(d.device), "hipSetDevice"))) break;
    if ((rc = upload(&d.quant_mem, &d.quant_leaf_base, tab.leaf_base, &d.bytes)) ||
        (rc = upload(&d.quant_mem, &d.quant_values, tab.values, &d.bytes)) ||
        (rc = upload(&d.quant_mem, &d.quant_weights, tab.weights, &d.bytes)))
      break;
  }
  if (rc) {
    const std::string err = g_last_error;
    for (size_t i = 0; i < f->devs.size(); ++i) {
      (void)hipSetDevice(f->devs[i]->device);
      free_quantile(*f->devs[i]);
      f->devs[i]->bytes = bytes0[i];
    }
    (void)hipGetLastError();
    (void)hipSetDevice(dev0);
    return fail(rc, err);
  }
  TI_HIP(hipSetDevice(dev0));
  f->quant_tab.reset();
  f->quant_ready.store(true, std::memory_order_release);
  return TI_OK;
}

}  // namespace
