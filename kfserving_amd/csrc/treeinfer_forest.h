// treeinfer_forest.h -- what a forest is on the host and on a device: the
// named layouts, the structs of libtreeinfer's host side (DeviceForest,
// HostImage, ti_forest) and the small helpers they need (errors, knobs,
// node words, upload).  Included by treeinfer.hip alone.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <utility>
#include <type_traits>
#include <vector>

#include "treeinfer.h"
#include "treeinfer_kernels.h"
#include "treeinfer_dispatch.h"
#include "treeinfer_linear.h"

using ti::ExpNode;
using ti::HeapNode;
using ti::KArgs;
using ti::KernelFn;

namespace ti {
struct ApproxLeaf;   // treeinfer_approx.h
}

// ---------------------------------------------------------- TreeSHAP paths
// Every root-to-leaf path of every tree, with the splits on one feature
// merged into one element (the unique path xgboost's TreeShap keeps: a
// feature seen again is unwound and re-extended at the end, so elements are
// in order of last occurrence).  An element holds the product of the
// child/parent cover ratios of its splits (zero fraction) and the condition
// a row must meet to follow all of them (one fraction 1, else 0): an interval
// with the NaN / zero flags for its numerical splits and, under kShapCat, a
// set of category codes for its LightGBM categorical splits (ShapCatRef).
struct ShapPath {
  int32_t group;    // output group (leaf_width 1)
  int32_t n;        // elements (excluding the root's dummy element)
  int64_t first;    // first element
  int64_t leaf;     // row of the path's leaf in the leaf-value table
};
constexpr uint32_t kShapNanOk = 1u;    // NaN follows every split of the element
constexpr uint32_t kShapZeroOk = 2u;   // exact 0 follows every split (LightGBM zero rule)
constexpr uint32_t kShapEmpty = 4u;    // no non-NaN value follows (a left turn at a NaN threshold)
constexpr uint32_t kShapCat = 8u;      // some split of the element is categorical: the row must
                                       //   also pass the set test (shap_cat_refs[element])
constexpr uint32_t kShapCatOutside = 16u;   // a value no bit of the set covers follows (NaN,
                                       //   x <= -1, x >= 2^31, a code past the last word): the
                                       //   path turns right at every categorical split
struct ShapElem {
  int32_t feature;
  uint32_t flags;
  double lo;        // follows iff !(x <= lo) && x <= hi (non-NaN, non-zero x); NaN: no lower
                    //   bound, so that -inf follows a path that only turns left on the feature
  double hi;
  double zf;        // zero fraction
};
static_assert(sizeof(ShapElem) == 32, "ShapElem is scalar-loaded as 32 bytes");
// The category set `allow` of a kShapCat element: words [first, first +
// nwords) of the forest's shap_cat_words; bit v % 32 of word v / 32 set iff
// code v follows every categorical split of the element.  One per element
// (zeros where kShapCat is clear), in forests with categorical nodes only.
struct alignas(8) ShapCatRef {   // one 8-byte scalar load
  uint32_t first;
  uint32_t nwords;
};

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int fail_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return TI_OK;
  return fail(TI_ERR_DEVICE, std::string(what) + " failed: " + hipGetErrorString(e));
}

#define TI_HIP(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(TI_ERR_DEVICE, std::string(#expr) + " failed: " + hipGetErrorString(e_)); \
  } while (0)

constexpr int kMaxHeapDepth = 8;              // deeper forests use the explicit layout
constexpr size_t kLdsPerCu = 160 * 1024;      // gfx950
constexpr size_t kFeatLdsMax = 64 * 1024;     // feature image budget per workgroup

// Environment knobs.  The layout / kernel A/B switches (TI_FORCE_LAYOUT,
// TI_TX_TOP, TI_LX_ILP, ...) are developer knobs, read only when
// TI_DEV_KNOBS=1: a serving worker that inherits a stray variable runs the
// default kernels (the reference plugin's one knob is
// nthread, python/xgbserver/xgbserver/model.py:38).  The operational settings
// below are always read; they change speed or memory, never the kernel or the
// results, and the per-forest ones are also ti_forest_set_option's.
bool dev_knobs() {
  const char* v = std::getenv("TI_DEV_KNOBS");
  return v && std::atoi(v) == 1;
}

bool operational_knob(const char* name) {
  static const char* const kOps[] = {"TI_CHUNK_MB", "TI_SHAP_TABLE_ROWS", "TI_SHAP_TABLE_MB"};
  for (const char* k : kOps)
    if (std::strcmp(k, name) == 0) return true;
  return false;
}

const char* env_knob(const char* name) {
  if (!operational_knob(name) && !dev_knobs()) return nullptr;
  const char* v = std::getenv(name);
  return v && *v ? v : nullptr;
}

int env_int(const char* name, int dflt) {
  const char* v = env_knob(name);
  return v ? std::atoi(v) : dflt;
}

// Rows per tile (= threads per workgroup) for a feature image of F columns
// of `xs`-byte elements: the largest of 256/128/64 whose [F][R] image fits
// kFeatLdsMax; 0 when even 64 rows do not fit (features read from HBM).
// (512-row tiles measured 25 % slower at F = 28: the bigger image leaves
// room for fewer workgroups per CU.)
int pick_rows(int F, size_t xs, int want) {
  if (want > 0) return want;
  for (int R = 256; R >= 64; R >>= 1)
    if (static_cast<size_t>(F) * R * xs <= kFeatLdsMax) return R;
  return 0;
}

size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

float round_down_f32(double t) {
  if (std::isnan(t)) return NAN;
  float f = static_cast<float>(t);
  if (static_cast<double>(f) > t) f = std::nextafter(f, -INFINITY);
  return f;
}

uint32_t make_meta(int32_t feature, uint8_t flags) {
  uint32_t m = static_cast<uint32_t>(feature) & ti::kMetaFeatMask;
  if (flags & TI_NODE_NAN_LEFT) m |= ti::kMetaNanLeft;
  if (flags & TI_NODE_ZERO_FLIP) m |= ti::kMetaZeroFlip;
  return m;
}

// a categorical node's meta (layouts 1 and 10): LightGBM's rule reads no flag;
// XGBoost's keeps the default child in the NaN bit
uint32_t make_cat_meta(uint32_t feature_field, uint8_t flags) {
  uint32_t m = (feature_field & ti::kMetaFeatMask) | ti::kMetaCat;
  if (flags & TI_NODE_CAT_XGB) {
    m |= ti::kMetaCatXgb;
    if (flags & TI_NODE_NAN_LEFT) m |= ti::kMetaNanLeft;
  }
  return m;
}

// padded heap node below a shallow leaf: always left (x <= +inf, NaN left)
constexpr uint32_t kPadMeta = ti::kMetaNanLeft;

// ---------------------------------------------------------------- layouts
// The device layouts, with the numbers ti_forest_info.layout reports
// (include/treeinfer.h; bench.py and the tests compare them).  2, 4 and 5 are
// retired.
enum Layout : int32_t {
  kLayoutHeap = 0,        // complete trees staged in LDS, float compares
  kLayoutExplicit = 1,    // explicit nodes, float compares (categorical splits too)
  kLayoutBinHeap = 3,     // binned heap: rank-binned features, 4-byte nodes
  kLayoutRecord = 6,      // record explicit: 8-byte slots, gathered
  kLayoutStaged = 7,      //   the same records, staged in LDS whole trees at a time
  kLayoutHeapTop = 8,     //   heap tops in LDS, the rest gathered
  kLayoutTopStaged = 9,   //   heap top + bottom, staged whole trees at a time
  kLayoutCatHeap = 10,    // categorical heap (the heap's fields)
};
// the record family: binned features, rx[] plans, the leaf tables of layout 1
constexpr bool is_record(int32_t l) { return l >= kLayoutRecord && l <= kLayoutTopStaged; }
// a heap top of hx_top levels in LDS
constexpr bool has_heap_top(int32_t l) { return l == kLayoutHeapTop || l == kLayoutTopStaged; }
// whole trees staged in LDS: lx_stage / lx_stage_cap / lx_ilp / n_stages
constexpr bool stages_trees(int32_t l) { return l == kLayoutStaged || l == kLayoutTopStaged; }
// the heap's fields: stride32/64, rows32/64, heap32/64 images
constexpr bool heap_fields(int32_t l) { return l == kLayoutHeap || l == kLayoutCatHeap; }

// What one group of device buffers allocated, in hipMalloc order.  A buffer is
// named where it is declared, packed and uploaded; freeing goes through here.
struct DeviceAllocs {
  std::vector<void*> ptrs;
  void release() {   // the buffers' device is current
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
};

// One device array: allocate, record it in `mem`, copy, count the bytes.  An
// empty source leaves a null pointer.  D is T, or void for the ACC-typed byte
// images.
template <typename D, typename T>
int upload(DeviceAllocs* mem, D** dst, const std::vector<T>& src, int64_t* bytes) {
  static_assert(std::is_void<D>::value || std::is_same<D, T>::value, "upload: pointer type");
  *dst = nullptr;
  if (src.empty()) return TI_OK;
  const size_t n = src.size() * sizeof(T);
  void* p = nullptr;
  TI_HIP(hipMalloc(&p, n));
  mem->ptrs.push_back(p);
  *dst = static_cast<D*>(p);
  TI_HIP(hipMemcpy(p, src.data(), n, hipMemcpyHostToDevice));
  *bytes += static_cast<int64_t>(n);
  return TI_OK;
}

// The forest's arrays on one device: what plan_launch reads.
struct ForestPtrs {
  // heap layout: one record per tree, float32-input and float64-input flavours
  unsigned char* heap32 = nullptr;
  unsigned char* heap64 = nullptr;
  int32_t* heap_leaf_ids = nullptr;
  // explicit layout
  ExpNode* nodes = nullptr;
  double* thr64 = nullptr;
  int64_t* node_base = nullptr;
  int32_t* root = nullptr;
  int64_t* leaf_base = nullptr;
  void* leaves = nullptr;
  int32_t* exp_leaf_ids = nullptr;
  uint32_t* cat_words = nullptr;
  int32_t* tree_group = nullptr;
  // binned heap layout: one image + threshold tables per input dtype
  unsigned char* bh_img[2] = {nullptr, nullptr};
  unsigned char* bh_fix_img = nullptr;   // the fixed walk's permuted image (fix_permute)
  unsigned char* bh_tbl[2] = {nullptr, nullptr};
  // record layouts (6-9): rank tables per input dtype
  unsigned char* bx_tbl[2] = {nullptr, nullptr};
  // record explicit layout
  uint2* rx_recs[2] = {nullptr, nullptr};
  uint32_t* rx_base = nullptr;
  uint32_t* rx_nint = nullptr;
  int32_t* lx_stage = nullptr;   // staged layouts (7, 9): first tree of each stage
  uint32_t* tx8_pos = nullptr;   // layout 9 compact bottom: first position of each tree
  void* tx8_val = nullptr;       //   leaf value per bottom position (ACC)
  int32_t* tx8_ord = nullptr;    //   leaf ordinal per bottom position
  uint32_t* hx_top[2] = {nullptr, nullptr};   // heap tops of layouts 8 and 9, per input dtype
  // linear leaves (treeinfer_linear.h): leaf records, their terms, first record of each tree
  ti::LinLeaf* lin_leaves = nullptr;
  ti::LinTerm* lin_terms = nullptr;
  int64_t* lin_leaf_base = nullptr;
  // pre-steps (treeinfer_pre.h): op codes [S] and constants [S * F]
  int32_t* pre_op = nullptr;
  double* pre_const = nullptr;
};

// TreeSHAP path tables (ensure_shap) and coefficient table (ensure_shap_table)
struct ShapPtrs {
  ShapPath* shap_paths = nullptr;
  ShapElem* shap_elems = nullptr;
  double* shap_leaf = nullptr;
  double* shap_bias = nullptr;
  ShapCatRef* shap_cat_refs = nullptr;   // [elements], forests with categorical nodes only
  uint32_t* shap_cat_words = nullptr;    //   the elements' category sets
  void* shap_tab = nullptr;          // TreeSHAP coefficient table (shap_table_kernel), MT-typed
  int64_t* shap_tab_off = nullptr;   // [paths] first coefficient of each path
};

// Approximate-contribution tables (treeinfer_approx.h: ensure_approx)
struct ApproxPtrs {
  int64_t* approx_leaf_base = nullptr;       // [T + 1] first leaf record of each tree
  ti::ApproxLeaf* approx_leaves = nullptr;   // per (tree, leaf id) {begin, count}
  void* approx_terms = nullptr;              // {delta, column}, float or double deltas
  double* approx_bias = nullptr;             // [K]
};

// ti_predict scratch: device buffers + pinned host staging (grown x2)
struct ScratchBufs {
  void* x_buf = nullptr;
  size_t x_cap = 0;
  void* out_buf = nullptr;
  size_t out_cap = 0;
  void* hx_pin = nullptr;
  size_t hx_cap = 0;
  void* ho_pin = nullptr;
  size_t ho_cap = 0;
  // the chunk pipeline of batches larger than one chunk (predict_shard): two
  // lanes, each a stream with its own pinned and device buffers
  hipStream_t lane_stream[2] = {nullptr, nullptr};
  void* lane_hx[2] = {nullptr, nullptr};
  void* lane_ho[2] = {nullptr, nullptr};
  void* lane_dx[2] = {nullptr, nullptr};
  void* lane_do[2] = {nullptr, nullptr};
  size_t lane_x_cap = 0, lane_o_cap = 0;
};

// The scratch of calls in flight on one replica (launch_chunked's part columns,
// TreeSHAP's slice partials and accumulator, the leaf ids of the linear and
// approximate passes): hipMalloc buffers of the replica's own, taken for a
// call and given back behind its last kernel with an event.  A call takes a
// buffer whose event has completed, or one given back on the call's own
// stream, and makes its stream wait for that event either way (a wait that
// orders nothing new, unless a new stream got a destroyed one's handle);
// otherwise it gets another buffer, so calls on different streams (the host
// pipeline's lanes, a caller's streams) never wait for each other.  Buffers
// grow to the size asked for, rounded up to 64 KiB, never shrink, and are
// freed with the replica; growing one frees and allocates device memory,
// which may synchronise the device.  Not the runtime's stream-ordered pool
// (hipMallocAsync): on the HIP 7.2 runtime its blocks came back to later calls
// of other sizes while still holding live data ("Call scratch").
struct CallScratch {
  struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;     // recorded when the buffer was given back
    hipStream_t last = nullptr;    // on this stream
    bool held = false;
  };
  std::mutex mu;
  std::vector<Buf> bufs;
};

// One replica.  Four groups of device memory, each a plain aggregate of
// pointers (bases, so d.heap32 reads as before) reset by one assignment: the
// forest's arrays, the TreeSHAP tables and the approximate-contribution
// tables, freed from the record of what their uploads allocated (forest_mem /
// shap_mem / approx_mem), and the scratch buffers, which grow() reallocates and
// free_scratch frees.
struct DeviceForest : ForestPtrs, ShapPtrs, ApproxPtrs, ScratchBufs {
  int device = -1;
  hipStream_t stream = nullptr;
  DeviceAllocs forest_mem, shap_mem, approx_mem;
  std::atomic<int32_t> shap_tab_state{0};   // 0 not tried, 1 built, -1 failed or over the cap:
                                     // contributions use the extend / unwind kernel
  // TI_OUTPUT_INTERACT scratch (launch_interact: contributions + partials of
  // one call): grow-only device memory of the replica's own, handed from one
  // call to the next, whatever their streams, through interact_done
  std::mutex interact_mu;
  void* interact_buf = nullptr;
  size_t interact_cap = 0;
  hipEvent_t interact_done = nullptr;
  CallScratch scratch;
  int64_t bytes = 0;
  std::mutex mu;
};

// A buffer of at least `bytes` for work enqueued on `stream` (device current),
// or nullptr when the device has no memory for it.
inline void* scratch_take(DeviceForest& d, size_t bytes, hipStream_t stream) {
  std::lock_guard<std::mutex> lk(d.scratch.mu);
  bytes = (std::max<size_t>(bytes, 1) + 65535) & ~size_t(65535);
  CallScratch::Buf* pick = nullptr;
  for (auto& b : d.scratch.bufs) {
    if (b.held) continue;
    const bool done = hipEventQuery(b.done) == hipSuccess;   // never recorded: done
    if (!done) (void)hipGetLastError();
    // one that fits, the smallest such; else one to regrow, which must be
    // idle on the device (the largest such)
    if (b.cap >= bytes ? !(done || b.last == stream) : !done) continue;
    if (!pick || (b.cap >= bytes ? (pick->cap < bytes || b.cap < pick->cap)
                                 : (pick->cap < bytes && b.cap > pick->cap)))
      pick = &b;
  }
  if (!pick) {
    CallScratch::Buf b;
    if (hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    d.scratch.bufs.push_back(b);
    pick = &d.scratch.bufs.back();
  }
  if (pick->cap < bytes) {
    // its event has completed, so nothing reads or writes it; hipFree and
    // hipMalloc may still synchronise the device (ti_predict_device's note)
    if (pick->p) (void)hipFree(pick->p);
    pick->p = nullptr;
    pick->cap = 0;
    if (hipMalloc(&pick->p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      pick->p = nullptr;
      return nullptr;
    }
    pick->cap = bytes;
  } else {
    (void)hipStreamWaitEvent(stream, pick->done, 0);
  }
  pick->held = true;
  pick->last = stream;
  return pick->p;
}

inline void scratch_give(DeviceForest& d, void* p, hipStream_t stream) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(d.scratch.mu);
  for (auto& b : d.scratch.bufs)
    if (b.p == p) {
      (void)hipEventRecord(b.done, stream);
      b.last = stream;
      b.held = false;
    }
}

// One scratch buffer for the scope of a call: given back, behind whatever the
// call enqueued on the stream, when the scope ends on any path.
struct ScratchHold {
  DeviceForest& d;
  hipStream_t s;
  void* p = nullptr;
  ScratchHold(DeviceForest& d_, hipStream_t s_) : d(d_), s(s_) {}
  ScratchHold(const ScratchHold&) = delete;
  ScratchHold& operator=(const ScratchHold&) = delete;
  bool take(size_t bytes) {
    p = scratch_take(d, bytes, s);
    return p != nullptr;
  }
  void give() {
    scratch_give(d, p, s);
    p = nullptr;
  }
  ~ScratchHold() { give(); }
};

// Binned heap layout (3): one image per input dtype (the ranks differ: float32
// view round_down_f32(t), float64 view t).  BinPlan is what the launch plan
// reads and stays in the forest; BinImage adds the packed bytes (HostImage).
struct BinPlan {
  int32_t L = 0;
  int32_t kary = 0;                 // > 0: tbl holds float32 5-ary tables of this height
  int32_t bkt_nb = 0;               // > 0: tbl holds float32 bucket tables of this many buckets
  int32_t b16 = 1;
  int32_t rows = 256;
  int32_t words = 0;                // packed bin words per row
  int64_t stride = 0;
  uint32_t mask = ti::kBNodeOffMask;   // bin-offset bits of a node word
};
struct BinImage : BinPlan {
  std::vector<unsigned char> img;   // [T][stride]
  std::vector<unsigned char> fix_img;   // img with hot pair slots first (fix_permute), or empty
  std::vector<unsigned char> tbl;   // [F][2^L] XT Eytzinger tables, 5-ary (kary > 0) or
                                    // bucket tables (bkt_nb > 0)
};

// Record explicit layout (6): 8-byte slots per input dtype (ranks differ),
// shared per-tree first slot, per-slot leaf values / ids.  RecPlan / RecExplicit
// as BinPlan / BinImage.
struct RecPlan {
  int32_t L = 0;
  int32_t rows = 256;
  int32_t words = 0;
  int32_t kary = 0;            // > 0: tbl holds 5-ary search tables of this height
  int32_t b8 = 0;              // u8 bins (layout 9 only; RxBins<true> in the kernels)
};
struct RecExplicit : RecPlan {
  std::vector<uint2> recs;
  std::vector<unsigned char> tbl;
  std::vector<uint32_t> top;   // heap tops (layout 8): [T][2^(hx_top+1)] u32;
                               // layout 9: per tree [top | bottom]
};

// The arrays a record-family planner fills (RecCandidate in treeinfer_pack.h)
// and the host image keeps.
struct RecArrays {
  RecExplicit rx[2];   // one view per input dtype
  // staged layouts (7, 9): stage k holds trees [lx_stage[k], lx_stage[k+1])
  std::vector<int32_t> lx_stage;
  // layout 9: per tree [top | bottom] in rx[i].top, tree byte offsets [T+1]
  // and bottom internal counts [T]
  std::vector<uint32_t> tx_off, tx_nint;
  // layout 9's compact bottom (plan_tx8): per tree the first bottom position
  // [T+1], and per bottom position the leaf value (ACC) / ordinal
  std::vector<uint32_t> tx8_pos;
  std::vector<unsigned char> tx8_val;
  std::vector<int32_t> tx8_ord;
};

// Every packed array that exists only to be uploaded.  The forest owns one
// until its last replica is resident (ti_forest_create), then drops it whole.
struct HostImage {
  std::vector<int32_t> group;   // [T] output group of each tree
  // heap layouts (0, 10); heap_leaf_ids also the binned heap's (3)
  std::vector<unsigned char> heap32, heap64;
  std::vector<int32_t> heap_leaf_ids;
  BinImage bh[2];
  // explicit layout (1); leaf_base / leaves / exp_leaf_ids also the record layouts'
  std::vector<ExpNode> nodes;
  std::vector<double> thr64;
  std::vector<int64_t> node_base, leaf_base;
  std::vector<int32_t> root, exp_leaf_ids;
  std::vector<uint32_t> cat_words;   // [nwords, w0, w1, ...] per categorical node
  std::vector<unsigned char> leaves;   // ACC-typed
  std::vector<int64_t> exp_src;   // explicit internal node -> descriptor node
  // record layouts (6-9)
  RecArrays rec;
  std::vector<uint32_t> rx_base, rx_nint;   // rx_base: [T+1]
  // linear leaves (ABI 6): per tree the first leaf record, per (tree, library
  // leaf id) a record, per term a 16-byte {coefficient, feature}
  std::vector<ti::LinLeaf> lin_leaves;
  std::vector<ti::LinTerm> lin_terms;
  std::vector<int64_t> lin_leaf_base;
  // pre-steps (ABI 9): the descriptor's op codes [S] and constants [S * F]
  std::vector<int32_t> pre_op;
  std::vector<double> pre_const;
};

}  // namespace

// Three lifetimes: the model's scalars (fill_model), the chosen layout's plan
// scalars (choose_layout; what plan_launch, tile_for, bheap_fixed,
// heap_stage_trees and ti_forest_get_info read), and the host image, which
// lives until upload.  The TreeSHAP source and tables have their own lazy
// lifecycle (keep_shap_source, ensure_shap).
struct ti_forest {
  // Forests with more than kMaxGroups outputs are split into parts of at most
  // kMaxGroups groups each (see create_chunked); the parent holds the parts.
  std::vector<std::unique_ptr<ti_forest>> parts;
  std::vector<int32_t> part_k0;                  // first output group of each part
  std::vector<std::vector<int32_t>> part_trees;  // original tree index of each part tree
  // ---- the model (fill_model)
  int32_t T = 0, F = 0, K = 1, LW = 1, accum = TI_F32, base_first = 1, lgb_zero_map = 0;
  int32_t zero_rule = 0, transform = TI_TRANSFORM_IDENTITY;
  double tparam = 1.0, divisor = 1.0;
  double base[ti::kMaxGroups] = {0};
  int32_t depth = 0;
  int32_t has_cat = 0;       // some split is categorical ...
  int32_t has_cat_xgb = 0;   // ... with XGBoost's rule (TI_NODE_CAT_XGB)
  int32_t has_cat_lgb = 0;   // ... with LightGBM's rule
  int32_t linear = 0;        // linear leaves (ABI 6; pack_linear)
  // pre-steps (ABI 9) this forest applies where X enters (launch_any).  A
  // forest split into group parts applies them itself, once, with the arrays
  // its first part's replicas hold; the parts apply none.
  int32_t pre_steps = 0;
  // ---- the layout's plan (choose_layout)
  int32_t layout = kLayoutHeap;
  int64_t stride32 = 0, stride64 = 0;
  int32_t rows32 = 256, rows64 = 256;   // heap: rows per tile of each image (0 = HBM features)
  BinPlan bh[2];
  RecPlan rx[2];
  int64_t rx_slots = 0;
  int32_t rx_ilp = 8;
  // staged layouts (7, 9): whole trees copied into LDS a stage at a time
  int32_t n_stages = 0;
  int64_t lx_stage_cap = 0;    // LDS bytes of the stage area
  int32_t lx_ilp = 8;
  // heap top + record bottom (layout 8): the top hx_top levels of each tree
  // staged in LDS hx_stage trees at a time, walked hx_ilp trees per lane
  // (hx_top also layout 9's top depth)
  int32_t hx_top = 0, hx_stage = 0, hx_ilp = 8;
  int32_t tx8 = 0;                 // 1: compact u8 bottom, 2: compact u16 bottom, 3: the u16
                                   //   bottom walked two lanes a row (t16split_predict_kernel)
  uint32_t tx16_mask = 0;          //   u16: the bottom word's bin-offset bits (KArgs bin_mask)
  // ---- the packed arrays, until every replica is resident
  std::unique_ptr<HostImage> host;
  // TreeSHAP (TI_OUTPUT_CONTRIB); has_shap = 0 when the forest has no covers
  // (shap_refused = 1) or a categorical node with XGBoost's rule (2).
  // The path tables are built and uploaded on the first contributions call
  // (ensure_shap), from a host copy of the arrays they need, so predict-only
  // serving never pays for them.
  int32_t has_shap = 0, shap_refused = 0, shap_maxl = 0;
  int64_t shap_npaths = 0;
  std::atomic<bool> shap_ready{false};
  std::mutex shap_mu;
  struct ShapSource {
    ti_forest_desc desc;
    std::vector<int64_t> tree_offset;
    std::vector<int32_t> tree_group, feature, left, right;
    std::vector<double> threshold, leaf_value, base_margin, cover;
    std::vector<uint8_t> flags;
    std::vector<uint32_t> cat_bits;      // all n_cat_words (a tree subset keeps them whole)
    std::vector<int64_t> cat_offset;
    std::vector<int32_t> cat_nwords;
  };
  std::unique_ptr<ShapSource> shap_src;
  std::vector<ShapPath> h_paths;
  // TreeSHAP coefficient table: per path, (2^n one-patterns) x n coefficients
  // (contrib_reg_kernel TAB); shap_tab_mt = 4 / 8 bytes per coefficient, 0: the
  // forest's paths cannot use one.  Built per replica on the first
  // contributions batch of at most shap_tab_rows rows, if its bytes stay under
  // shap_tab_mb (ti_forest_set_option; defaults $TI_SHAP_TABLE_ROWS /
  // $TI_SHAP_TABLE_MB read at ti_forest_create); optional: a failed build
  // leaves the extend / unwind kernel in charge.
  int32_t shap_tab_mt = 0;
  std::vector<int64_t> h_tab_off;
  int64_t shap_tab_len = 0;
  int64_t shap_tab_rows = env_int("TI_SHAP_TABLE_ROWS", 16384);
  int64_t shap_tab_mb = env_int("TI_SHAP_TABLE_MB", 1280);
  // TI_OPT_HOST_REGISTER (developer default: $TI_HOST_REGISTER under TI_DEV_KNOBS)
  std::atomic<int32_t> host_register{env_int("TI_HOST_REGISTER", 0) != 0 ? 1 : 0};
  double shap_tab_build_ms = 0.0;   // the last table build (slot's shap_table_kernel + upload)
  std::vector<ShapElem> h_elems;
  std::vector<ShapCatRef> h_shap_cat_refs;   // parallel to h_elems, or empty
  std::vector<uint32_t> h_shap_cat;          // the category sets of all paths
  std::vector<double> h_path_leaf, h_shap_bias;
  std::atomic<int64_t> lin_scratch_mb{1024};   // TI_OPT_LINEAR_SCRATCH_MB
  // Approximate contributions (TI_OUTPUT_CONTRIB_APPROX, treeinfer_approx.h):
  // approx_refused = 1 without covers, 2 with linear leaves.  The tables are
  // built and uploaded on the first call (ensure_approx, under shap_mu) from
  // this host copy of the arrays they read, which goes once they are resident.
  int32_t approx_refused = 0;
  std::atomic<bool> approx_ready{false};
  struct ApproxSource {
    std::vector<int64_t> tree_offset;
    std::vector<int32_t> tree_group, feature, left, right, leaf_id;
    std::vector<double> leaf_value, cover, base_margin;
  };
  std::unique_ptr<ApproxSource> approx_src;
  std::vector<std::unique_ptr<DeviceForest>> devs;
};
