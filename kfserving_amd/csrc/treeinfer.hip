// treeinfer.hip — libtreeinfer.so: C ABI (include/treeinfer.h) over the
// gfx950 kernels in treeinfer_kernels.h.
//
// Host responsibilities:
//   * validate the canonical SoA forest handed over by the Python loaders
//     (kfserving_amd/formats/*), which replaces the library handles built in
//     xgbserver/model.py:38-39, lgbserver/model.py:39-40,
//     sklearnserver/model.py:38, choose a device layout and pack it
//     (treeinfer_pack.h; the structs and the named layouts: treeinfer_forest.h);
//   * here: upload one replica per device and free it, plan and launch the
//     predict kernels, the host pipelines and the C ABI (TreeSHAP:
//     treeinfer_shap.h);
//   * ti_predict: shard rows in contiguous blocks over the devices (one host
//     thread per device, one stream each), H2D -> one fused kernel -> D2H.
//     This replaces XGBoosterPredict / LGBM_BoosterPredictForMat /
//     Forest*.predict at xgbserver/model.py:46-47, lgbserver/model.py:51,
//     sklearnserver/model.py:50.
#include <hip/hip_runtime.h>

#include "treeinfer_forest.h"
#include "treeinfer_pack.h"
#include "treeinfer_shap.h"
#include "treeinfer_approx.h"
#include "treeinfer_pre.h"

namespace {

// the scratch and staging buffers of one replica (device current)
void free_scratch(DeviceForest& d) {
  if (d.x_buf) (void)hipFree(d.x_buf);
  if (d.out_buf) (void)hipFree(d.out_buf);
  if (d.hx_pin) (void)hipHostFree(d.hx_pin);
  if (d.ho_pin) (void)hipHostFree(d.ho_pin);
  for (int l = 0; l < 2; ++l) {
    if (d.lane_hx[l]) (void)hipHostFree(d.lane_hx[l]);
    if (d.lane_ho[l]) (void)hipHostFree(d.lane_ho[l]);
    if (d.lane_dx[l]) (void)hipFree(d.lane_dx[l]);
    if (d.lane_do[l]) (void)hipFree(d.lane_do[l]);
    if (d.lane_stream[l]) (void)hipStreamDestroy(d.lane_stream[l]);
  }
  static_cast<ScratchBufs&>(d) = ScratchBufs();
}

void free_device(DeviceForest& d) {
  if (d.device < 0) return;
  (void)hipSetDevice(d.device);
  d.forest_mem.release();
  static_cast<ForestPtrs&>(d) = ForestPtrs();
  free_shap(d);
  free_approx(d);
  free_scratch(d);
  if (d.interact_done) (void)hipEventDestroy(d.interact_done);
  if (d.interact_buf) (void)hipFree(d.interact_buf);
  d.interact_done = nullptr;
  d.interact_buf = nullptr;
  d.interact_cap = 0;
  for (auto& b : d.scratch.bufs) {
    if (b.done) (void)hipEventDestroy(b.done);
    if (b.p) (void)hipFree(b.p);
  }
  d.scratch.bufs.clear();
  if (d.stream) (void)hipStreamDestroy(d.stream);
  d.stream = nullptr;
  d.device = -1;
}

// One replica: which arrays each layout uploads, in hipMalloc order.
int upload_device(const ti_forest* f, DeviceForest& d, int device) {
  const HostImage& h = *f->host;
  const int32_t L = f->layout;
  d.device = device;
  TI_HIP(hipSetDevice(device));
  TI_HIP(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  int rc = TI_OK;
  // stops at the first failure; free_device frees what was recorded
  auto up = [&](auto** dst, const auto& src) {
    if (rc == TI_OK) rc = upload(&d.forest_mem, dst, src, &d.bytes);
  };
  up(&d.tree_group, h.group);
  if (heap_fields(L)) {
    up(&d.heap32, h.heap32);
    up(&d.heap64, h.heap64);
    up(&d.heap_leaf_ids, h.heap_leaf_ids);
  } else if (is_record(L)) {
    // 6-8 walk the records (8: below a heap top); 9 walks [top | bottom] images
    // and takes rx_base / rx_nint from the tx arrays
    const bool tx = L == kLayoutTopStaged;
    for (int i = 0; i < 2; ++i) {
      if (tx) up(&d.hx_top[i], h.rec.rx[i].top);
      else up(&d.rx_recs[i], h.rec.rx[i].recs);
      up(&d.bx_tbl[i], h.rec.rx[i].tbl);
      if (L == kLayoutHeapTop) up(&d.hx_top[i], h.rec.rx[i].top);
    }
    up(&d.rx_base, tx ? h.rec.tx_off : h.rx_base);
    up(&d.rx_nint, tx ? h.rec.tx_nint : h.rx_nint);
    if (tx && f->tx8) {
      up(&d.tx8_pos, h.rec.tx8_pos);
      up(&d.tx8_val, h.rec.tx8_val);
      up(&d.tx8_ord, h.rec.tx8_ord);
    }
    if (stages_trees(L)) up(&d.lx_stage, h.rec.lx_stage);
    up(&d.leaf_base, h.leaf_base);
    if (f->LW > 1) up(&d.leaves, h.leaves);   // vector leaves are read from the leaf table
    up(&d.exp_leaf_ids, h.exp_leaf_ids);
  } else if (L == kLayoutBinHeap) {
    for (int i = 0; i < 2; ++i) {
      up(&d.bh_img[i], h.bh[i].img);
      up(&d.bh_tbl[i], h.bh[i].tbl);
    }
    // the permuted image of the fixed walk (float32 view only): once per replica
    up(&d.bh_fix_img, h.bh[0].fix_img);
    up(&d.heap_leaf_ids, h.heap_leaf_ids);
  } else {
    up(&d.nodes, h.nodes);
    up(&d.thr64, h.thr64);
    up(&d.node_base, h.node_base);
    up(&d.root, h.root);
    up(&d.leaf_base, h.leaf_base);
    up(&d.leaves, h.leaves);
    up(&d.exp_leaf_ids, h.exp_leaf_ids);
    up(&d.cat_words, h.cat_words);
  }
  if (f->linear) {
    up(&d.lin_leaves, h.lin_leaves);
    up(&d.lin_terms, h.lin_terms);
    up(&d.lin_leaf_base, h.lin_leaf_base);
  }
  up(&d.pre_op, h.pre_op);
  up(&d.pre_const, h.pre_const);
  return rc;
}

// ----------------------------------------------------------------- launch
// plan_launch decides what does not depend on the batch -- tile rows, block,
// LDS bytes, the kernel's key and its arguments -- and launch() adds the batch
// and holds the one launch site of the predict kernels.  The kernels live in
// one translation unit per (input, accumulator) type pair (treeinfer_k_*.hip,
// compiled in parallel); ti::select finds one from its key (treeinfer_dispatch.h).

// Columns per pass of the record layouts' coalesced binning through the stage
// area (rx_stage_bins): a multiple of 8 that fits `bytes` for R rows, at most
// the features rounded up to 8; 0 (per-lane row loads) when fewer than 8 fit.
int32_t bin_chunk_for(size_t bytes, int R, int xdt, int F) {
  const size_t per_col = static_cast<size_t>(R) * (xdt == TI_F64 ? 8 : 4);
  size_t c = (bytes / per_col) & ~size_t(7);
  c = std::min(c, static_cast<size_t>((F + 7) & ~7));
  return c >= 8 ? static_cast<int32_t>(c) : 0;
}

std::mutex g_attr_mu;
std::set<std::pair<int, const void*>> g_attr_done;

// Once per (device, kernel): the kernels address LDS as offsets from 0, which
// holds only while they declare no static LDS -- check it, then raise the
// dynamic-LDS limit to the whole 160 KiB.
int ensure_lds_attr(int device, KernelFn fn) {
  std::lock_guard<std::mutex> lk(g_attr_mu);
  auto key = std::make_pair(device, reinterpret_cast<const void*>(fn));
  if (g_attr_done.count(key)) return TI_OK;
  hipFuncAttributes attr;
  TI_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(fn)));
  if (attr.sharedSizeBytes != 0)
    return fail(TI_ERR_DEVICE, "kernel declares " + std::to_string(attr.sharedSizeBytes) +
                                   " B of static LDS; the LDS-address-0 layout is violated");
  TI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsPerCu)));
  g_attr_done.insert(key);
  return TI_OK;
}

// TI_OCC=1: print, once per kernel, the workgroups per CU the runtime's
// occupancy calculator allows for this launch shape (a diagnostic for the
// PMC passes' resident-wave counts).
void occ_note(KernelFn fn, int block, size_t lds) {
  static const int on = env_int("TI_OCC", 0);
  if (!on) return;
  static std::mutex mu;
  static std::set<const void*> seen;
  std::lock_guard<std::mutex> lk(mu);
  if (!seen.insert(reinterpret_cast<const void*>(fn)).second) return;
  int n = -1;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(fn), block, lds);
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(fn));
  std::fprintf(stderr, "[ti occupancy] block %d lds %zu B: %d workgroups/CU (%d waves/SIMD), %d VGPRs, %d SGPRs\n",
               block, lds, n, n * ((block + 63) / 64) / 4, attr.numRegs, 0);
}

int64_t output_width(const ti_forest* f, int kind) {
  if (kind == TI_OUTPUT_LEAF) return f->T;
  if (kind == TI_OUTPUT_CONTRIB || kind == TI_OUTPUT_CONTRIB_APPROX)
    return static_cast<int64_t>(f->K) * (f->F + 1);
  if (kind == TI_OUTPUT_INTERACT) return static_cast<int64_t>(f->K) * (f->F + 1) * (f->F + 1);
  if (kind == TI_OUTPUT_PREDICT && f->transform == TI_TRANSFORM_ARGMAX) return 1;
  return f->K;
}

int output_dtype(const ti_forest* f, int kind) {
  if (kind == TI_OUTPUT_LEAF) return TI_I32;
  return f->accum;
}

size_t dtype_size(int dt) { return dt == TI_F64 ? 8 : 4; }

// Whether a binned-heap launch takes the fixed-layout walk (bheap_fix_kernel):
// float32 input and sums, one scalar leaf per leaf, depth-8 records of 2 KB,
// 512-row tiles (the node words carry their heap index) and at most 14 bin
// words (the image ends below kFixFlag); leaf ids keep the indexed walk.
// TI_BHEAP_FIX=0 turns it off.
bool bheap_fixed(const ti_forest* f, int xdt, int kind) {
  if (f->layout != kLayoutBinHeap || xdt != TI_F32 || f->accum != TI_F32 || f->LW != 1 || f->depth != 8)
    return false;
  if (kind != TI_OUTPUT_MARGIN && kind != TI_OUTPUT_PREDICT) return false;
  const BinPlan& bi = f->bh[0];
  return env_int("TI_BHEAP_FIX", 1) != 0 && bi.rows == ti::kFixRows && bi.mask == ti::kBNodeOffMask512 &&
         bi.stride == ti::kFixTree && static_cast<uint32_t>(bi.words) * 2048u <= ti::kFixFlag;
}

// Rows per tile and the LDS bytes of the feature (or bin) image, for batches
// of input type xdt.  The heap, binned and record images fixed R at create
// time (their meta words hold [F][R] byte offsets); the float explicit layout
// takes the largest R whose feature image fits.  !feat_lds: features stay in
// HBM, tiles of 256 rows.
struct Tile {
  int R;
  bool feat_lds;
  size_t feat_bytes;
};

Tile tile_for(const ti_forest* f, int xdt) {
  const size_t xs = dtype_size(xdt);
  const int ii = xdt == TI_F64 ? 1 : 0;
  const bool rec = is_record(f->layout);
  int R;
  if (heap_fields(f->layout)) {
    R = xdt == TI_F64 ? f->rows64 : f->rows32;
  } else if (f->layout == kLayoutBinHeap) {
    R = f->bh[ii].rows;
  } else if (rec) {
    R = f->rx[ii].rows;
  } else {
    R = 256;
    while (R > 64 && static_cast<size_t>(f->F) * R * xs > kFeatLdsMax) R >>= 1;
    if (static_cast<size_t>(f->F) * R * xs > kFeatLdsMax) R = 0;
  }
  Tile t;
  t.feat_lds = R > 0;
  t.R = t.feat_lds ? R : 256;
  t.feat_bytes = t.feat_lds ? align16(static_cast<size_t>(f->F) * t.R * xs) : 0;
  if (f->layout == kLayoutBinHeap) t.feat_bytes = static_cast<size_t>(f->bh[ii].words) * t.R * 4;
  if (rec) t.feat_bytes = static_cast<size_t>(f->rx[ii].words) * t.R * 4;
  return t;
}

// The same for a created heap forest and batches of input type xdt: what
// plan_launch stages and ti_forest_get_info reports.
int64_t heap_stage_trees(const ti_forest* f, int xdt) {
  const Tile t = tile_for(f, xdt);
  return heap_stage_trees(f, xdt == TI_F64 ? f->stride64 : f->stride32, t.feat_bytes + 16, t.R);
}

// Everything about a launch that does not depend on the batch.
struct LaunchPlan {
  ti::KernelKey key;
  int R;        // rows per tile
  int block;    // threads per workgroup: R, or 2R for the two-lane walk
  size_t lds;   // dynamic LDS bytes
  KArgs a;      // all but X, n_rows, row_stride, n_cols and out
};

// Plans the launch of forest f (device copy d) for batches of input type xdt
// and output `kind`.  Host arithmetic only: it makes no HIP call, and reads
// the knobs TI_BHEAP_FIX / TI_BHEAP_NG / TI_BIN_XPF (every call) and TI_HEAP_LDS_KB /
// TI_BHEAP_STAGE (once).
int plan_launch(const ti_forest* f, const DeviceForest& d, int xdt, int kind, LaunchPlan* p) {
  const size_t xs = dtype_size(xdt);
  const int ii = xdt == TI_F64 ? 1 : 0;
  const Tile t = tile_for(f, xdt);
  const int R = t.R;
  p->R = R;
  p->block = R;
  p->lds = t.feat_bytes + 16;   // feature image + NaN flag word

  ti::KernelKey& key = p->key;
  key = ti::KernelKey{};
  key.x64 = xdt == TI_F64;
  key.acc64 = f->accum == TI_F64;
  key.K = f->K;
  key.feat_lds = t.feat_lds;
  key.zero_rule = f->zero_rule != 0;

  KArgs& a = p->a;
  std::memset(&a, 0, sizeof(a));
  a.n_features = f->F;
  a.n_trees = f->T;
  a.n_groups = f->K;
  a.leaf_width = f->LW;
  a.kind = kind;
  a.transform = f->transform;
  a.base_first = f->base_first;
  a.lgb_zero_map = f->lgb_zero_map;
  a.divide = f->divisor != 1.0;
  a.transform_param = f->tparam;
  a.average_divisor = f->divisor;
  for (int k = 0; k < ti::kMaxGroups; ++k) a.base[k] = f->base[k];
  a.tree_group = d.tree_group;

  if (heap_fields(f->layout)) {
    // [feature image][flag][stage area = S tree records]
    const int64_t stride_b = xdt == TI_F64 ? f->stride64 : f->stride32;
    a.trees = xdt == TI_F64 ? d.heap64 : d.heap32;
    a.tree_stride = stride_b;
    a.heap_leaf_ids = d.heap_leaf_ids;
    a.depth = f->depth;
    const int64_t S = heap_stage_trees(f, xdt);
    if (S < 1) return fail(TI_ERR_UNSUPPORTED, "heap tree record does not fit in LDS");
    a.stage_trees = static_cast<int32_t>(S);
    p->lds += static_cast<size_t>(S * stride_b);
    key.walk = ti::Walk::Heap;
    if (f->layout == kLayoutCatHeap) {   // categorical heap: always an LDS feature image
      if (!t.feat_lds) return fail(TI_ERR_UNSUPPORTED, "categorical heap needs the LDS feature image");
      key.walk = f->has_cat_xgb != 0 ? ti::Walk::CatHeapXgb : ti::Walk::CatHeapLgb;
    }
  } else if (f->layout == kLayoutBinHeap) {
    // binned heap: [bin image][flag][stage area = S tree records, also the
    // binning temp of >= 8 columns].  S by grow_stage from kBTilp trees,
    // capped by the prefetch registers (PF x 16 B x R); unlike the heap
    // layouts no LDS-fit check, and TI_BHEAP_STAGE forces a size.
    const BinPlan& bi = f->bh[ii];
    const int64_t stride_b = bi.stride;
    const size_t fixed = align16(t.feat_bytes + 4);
    const size_t temp_min = 8 * static_cast<size_t>(R) * xs;
    auto area = [&](int64_t n) { return std::max(static_cast<size_t>(n * stride_b), temp_min); };
    const int64_t cap = static_cast<int64_t>(8) * 16 * R / stride_b;
    int64_t S = std::min<int64_t>(ti::kBTilp, cap);
    if (S < 1) return fail(TI_ERR_UNSUPPORTED, "binned heap tree record does not fit the stage");
    S = grow_stage(S, ti::kBTilp, cap, f->T, fixed, area);
    static const int force_s = env_int("TI_BHEAP_STAGE", 0);
    if (force_s > 0) S = std::min<int64_t>(force_s, cap);
    S = std::min<int64_t>(S, f->T);
    a.bin_mask = bi.mask;
    a.bin_kary = bi.kary;
    a.bin_nb = bi.bkt_nb;
    a.trees = d.bh_img[ii];
    a.tree_stride = stride_b;
    a.heap_leaf_ids = d.heap_leaf_ids;
    a.depth = f->depth;
    a.bin_tbl = d.bh_tbl[ii];
    a.bin_L = bi.L;
    a.bin_words = bi.words;
    key.bins16 = bi.b16 != 0;
    if (!bheap_fixed(f, xdt, kind)) {
      key.walk = ti::Walk::BinHeap;
      key.prefetch = S * stride_b <= static_cast<int64_t>(4) * 16 * R ? 4 : 8;
      const size_t ar = area(S);
      a.stage_trees = static_cast<int32_t>(S);
      a.stage_off = static_cast<int32_t>(fixed);
      a.bin_chunk = static_cast<int32_t>(std::min<size_t>((ar / (static_cast<size_t>(R) * xs)) & ~size_t(7),
                                                          static_cast<size_t>(f->F + 7) & ~size_t(7)));
      p->lds = fixed + ar;
    } else {
      // fixed layout (bheap_fix_kernel): [bins][flag][NG groups of 4 trees at
      // kFixStage]; the binning goes through the stage area, 4 NG columns at a
      // time.  NG = 1: 38,912 B, 4 workgroups (32 waves) per CU; where the
      // kernel takes its two-buffer loop (ti::fix_dma_path: one output group,
      // NG = 1, at least 8 trees) a second stage buffer: 47,104 B, 3 workgroups
      const int ng = std::min(2, std::max(1, env_int("TI_BHEAP_NG", 1)));
      const int kmax = f->K == 1 ? 1 : f->K <= 4 ? 4 : 16;   // with_k_zero's buckets
      key.walk = ti::Walk::BinHeapFixed;
      key.groups = ng;
      a.stage_trees = 4 * ng;
      a.bin_chunk = 4 * ng;
      a.bin_xpf = env_int("TI_BIN_XPF", 1) != 0;   // stage_bins' register path (NG = 1)
      a.stage_off = static_cast<int32_t>(ti::kFixStage);
      if (d.bh_fix_img != nullptr) a.trees = d.bh_fix_img;   // same walk, hot pair slots first
      p->lds = ti::fix_lds_bytes(kmax, ng, f->T);
    }
  } else if (is_record(f->layout)) {
    // record layouts: [bin image][flag][stage area (7, 8, 9)]
    const RecPlan& rx = f->rx[ii];
    a.rx_base = d.rx_base;   // 9: tree byte offsets in the image
    a.rx_nint = d.rx_nint;   // 9: bottom internal nodes
    a.leaf_base = d.leaf_base;
    a.leaves = d.leaves;
    a.exp_leaf_ids = d.exp_leaf_ids;
    a.bin_tbl = d.bx_tbl[ii];
    a.bin_L = rx.L;
    a.bin_kary = rx.kary;
    a.bin_words = rx.words;
    if (f->layout != kLayoutTopStaged) {
      a.rx_recs = d.rx_recs[ii];
      a.rx_slots = static_cast<uint32_t>(f->rx_slots);
    }
    if (has_heap_top(f->layout)) {   // heap top
      a.trees = reinterpret_cast<const unsigned char*>(d.hx_top[ii]);
      a.depth = f->hx_top;
    }
    if (f->layout != kLayoutRecord) a.stage_off = static_cast<int32_t>(align16(t.feat_bytes + 4));
    if (stages_trees(f->layout)) {   // stages of whole trees, at most lx_stage_cap bytes
      a.stage_start = d.lx_stage;
      a.n_stages = f->n_stages;
      p->lds = std::max(static_cast<size_t>(a.stage_off) + static_cast<size_t>(f->lx_stage_cap), kLxMinLds);
      if (p->lds > kLdsPerCu || static_cast<int64_t>(kLxPf) * 16 * R < f->lx_stage_cap)
        return fail(TI_ERR_UNSUPPORTED, f->layout == kLayoutStaged ? "staged record layout exceeds LDS"
                                                       : "heap-top staged layout exceeds LDS");
      a.bin_chunk = bin_chunk_for(static_cast<size_t>(f->lx_stage_cap), R, xdt, f->F);
    } else if (f->layout == kLayoutHeapTop) {   // stages of hx_stage heap tops
      a.tree_stride = static_cast<int64_t>(8) << f->hx_top;   // 2^(D0+1) u32
      a.stage_trees = f->hx_stage;
      p->lds = static_cast<size_t>(a.stage_off) + static_cast<size_t>(f->hx_stage) * a.tree_stride;
      if (p->lds > kLdsPerCu || static_cast<int64_t>(kHxPf) * 16 * R < f->hx_stage * a.tree_stride)
        return fail(TI_ERR_UNSUPPORTED, "heap-top layout exceeds LDS");
      a.bin_chunk = bin_chunk_for(static_cast<size_t>(f->hx_stage) * a.tree_stride, R, xdt, f->F);
    }
    if (f->layout == kLayoutTopStaged) {
      a.tx_pos = d.tx8_pos;
      a.tx_vals = d.tx8_val;
      a.tx_ord = d.tx8_ord;
      a.bin_mask = f->tx16_mask;
      key.walk = f->tx8 == 3 ? ti::Walk::BottomU16Split : f->tx8 == 2 ? ti::Walk::BottomU16
                 : f->tx8 ? ti::Walk::BottomU8 : ti::Walk::HeapTopStaged;
      key.bins16 = rx.b8 == 0;
      if (f->tx8 == 3) p->block = 2 * R;   // two lanes a row
    } else {
      key.walk = f->layout == kLayoutRecord ? ti::Walk::Record
                 : f->layout == kLayoutStaged ? ti::Walk::StagedRecord : ti::Walk::HeapTopRecord;
    }
    key.ilp = f->layout == kLayoutRecord ? f->rx_ilp : f->layout == kLayoutHeapTop ? f->hx_ilp : f->lx_ilp;
  } else {
    a.nodes = d.nodes;
    a.thr64 = d.thr64;
    a.node_base = d.node_base;
    a.root = d.root;
    a.leaf_base = d.leaf_base;
    a.leaves = d.leaves;
    a.exp_leaf_ids = d.exp_leaf_ids;
    a.cat_words = d.cat_words;
    key.walk = ti::Walk::Explicit;
  }
  return TI_OK;
}

// The one launch site of the predict kernels: the plan, the batch, the grid.
int launch(ti_forest* f, DeviceForest& d, const void* X, int xdt, int64_t rows, int32_t cols,
           int64_t stride, int kind, void* out, hipStream_t stream) {
  if (rows <= 0) return TI_OK;
  LaunchPlan p;
  int rc = plan_launch(f, d, xdt, kind, &p);
  if (rc) return rc;
  p.a.X = X;
  p.a.n_rows = rows;
  p.a.row_stride = stride;
  p.a.n_cols = cols;
  p.a.out = out;
  KernelFn fn = ti::select(p.key);
  rc = ensure_lds_attr(d.device, fn);
  if (rc) return rc;
  const int64_t grid = (rows + p.R - 1) / p.R;
  if (grid > 0x7fffffff) return fail(TI_ERR_INVALID, "too many rows for one launch");
  if (p.block != p.R && p.block > 512) return fail(TI_ERR_UNSUPPORTED, "two-lane walk needs tiles of <= 256 rows");
  occ_note(fn, p.block, p.lds);
  hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(grid)), dim3(p.block), p.lds, stream, p.a);
  TI_HIP(hipGetLastError());
  return TI_OK;
}

// Scratch buffers grow geometrically (x2, >= 4 MiB) so a serving process
// stops reallocating after its first few batch sizes.
int grow(void** buf, size_t* cap, size_t need, bool pinned = false) {
  if (need <= *cap) return TI_OK;
  const size_t n = std::max({need, static_cast<size_t>(4) << 20, 2 * *cap});
  if (*buf) (void)(pinned ? hipHostFree(*buf) : hipFree(*buf));
  *buf = nullptr;
  *cap = 0;
  if (pinned) {
    TI_HIP(hipHostMalloc(buf, n, hipHostMallocDefault));
  } else {
    TI_HIP(hipMalloc(buf, n));
  }
  *cap = n;
  return TI_OK;
}

int launch_any(ti_forest* f, int slot, const void* X, int xdt, int64_t rows, int32_t cols,
               int64_t stride, int kind, void* out, hipStream_t stream);
int launch_approx(ti_forest* f, DeviceForest& d, const void* X, int xdt, int64_t rows, int32_t cols,
                  int64_t stride, void* out, int64_t out_ld, hipStream_t stream);

// Host copies into / out of pinned staging: large copies split over threads
// (one thread moves ~10 GB/s from pageable memory; PCIe Gen5 x16 takes ~55).
void copy_parallel(void* dst, const void* src, size_t n) {
  constexpr size_t kPerThread = 8u << 20;
  const size_t want = std::min<size_t>(8, n / kPerThread);
  if (want < 2) {
    std::memcpy(dst, src, n);
    return;
  }
  std::vector<std::thread> th;
  const size_t part = (n / want + 63) & ~size_t(63);
  for (size_t i = 0; i < want; ++i) {
    const size_t lo = i * part;
    if (lo >= n) break;
    const size_t len = std::min(part, n - lo);
    th.emplace_back([=]() {
      std::memcpy(static_cast<unsigned char*>(dst) + lo, static_cast<const unsigned char*>(src) + lo, len);
    });
  }
  for (auto& t : th) t.join();
}

// Rows per chunk of the host pipeline: TI_CHUNK_MB (default 64) of input,
// a multiple of 512 rows (whole tiles).
int64_t chunk_rows(size_t row_bytes) {
  const int mb = env_int("TI_CHUNK_MB", 64);
  int64_t r = static_cast<int64_t>((static_cast<size_t>(std::max(mb, 1)) << 20) / std::max<size_t>(row_bytes, 1));
  r = std::max<int64_t>(512, r & ~int64_t(511));
  return r;
}

// The chunk of one call.  Every kind but TI_OUTPUT_INTERACT and
// TI_OUTPUT_CONTRIB_APPROX sizes it by the input row, as above.  An
// interaction row is K * (F + 1)^2 outputs, far wider than its input (C2:
// 3,364 B against 112 B), and the lanes hold a chunk of output as well: there
// TI_CHUNK_MB bounds the wider of the two rows, in whole 64-row waves (the
// interaction kernels have no 512-row tile).  Approximate contributions do the
// same with their K * (F + 1) outputs (their pass 2 has 64-row tiles too).
int64_t chunk_rows_for(const ti_forest* f, int xdt, int64_t stride, int kind) {
  const size_t x_row = static_cast<size_t>(stride) * dtype_size(xdt);
  if (kind != TI_OUTPUT_INTERACT && kind != TI_OUTPUT_CONTRIB_APPROX) return chunk_rows(x_row);
  const size_t o_row = dtype_size(output_dtype(f, kind)) * static_cast<size_t>(output_width(f, kind));
  const int mb = env_int("TI_CHUNK_MB", 64);
  const int64_t r = static_cast<int64_t>((static_cast<size_t>(std::max(mb, 1)) << 20) /
                                         std::max<size_t>(std::max(x_row, o_row), 1));
  return std::max<int64_t>(64, r & ~int64_t(63));
}

// Batches larger than one chunk: chunks alternate between two lanes (streams
// with their own pinned and device buffers).  While lane A runs chunk c
// (H2D -> kernel -> D2H), the host copies chunk c+1 into lane B's pinned
// buffer and enqueues it, so B's H2D overlaps A's kernel; before lane A takes
// chunk c+2 the host waits for chunk c and copies its result out.  Pinned
// memory is 2 x (chunk in + chunk out) whatever the batch size.
int predict_pipelined(ti_forest* f, int slot, DeviceForest& d, const unsigned char* X, int xdt,
                      int64_t rows, int32_t cols, int64_t stride, int kind, unsigned char* out,
                      int64_t ch) {
  const size_t xs = dtype_size(xdt);
  const size_t os = dtype_size(output_dtype(f, kind)) * output_width(f, kind);
  const size_t x_row = static_cast<size_t>(stride) * xs;
  const size_t x_cap = static_cast<size_t>(ch) * x_row;
  const size_t o_cap = static_cast<size_t>(ch) * os;
  // Whatever path leaves this function (an early TI_HIP return or a failed
  // launch included), no copy or kernel queued on a lane outlives it: the
  // next call reuses -- or frees -- the lane buffers that work reads and writes.
  struct LaneSync {
    DeviceForest& d;
    ~LaneSync() {
      for (int l = 0; l < 2; ++l)
        if (d.lane_stream[l]) (void)hipStreamSynchronize(d.lane_stream[l]);
    }
  } lane_sync{d};
  if (d.lane_x_cap < x_cap || d.lane_o_cap < o_cap) {
    for (int l = 0; l < 2; ++l) {
      if (d.lane_hx[l]) (void)hipHostFree(d.lane_hx[l]);
      if (d.lane_ho[l]) (void)hipHostFree(d.lane_ho[l]);
      if (d.lane_dx[l]) (void)hipFree(d.lane_dx[l]);
      if (d.lane_do[l]) (void)hipFree(d.lane_do[l]);
      d.lane_hx[l] = d.lane_ho[l] = d.lane_dx[l] = d.lane_do[l] = nullptr;
    }
    d.lane_x_cap = d.lane_o_cap = 0;
    for (int l = 0; l < 2; ++l) {
      TI_HIP(hipHostMalloc(&d.lane_hx[l], x_cap, hipHostMallocDefault));
      TI_HIP(hipHostMalloc(&d.lane_ho[l], o_cap, hipHostMallocDefault));
      TI_HIP(hipMalloc(&d.lane_dx[l], x_cap));
      TI_HIP(hipMalloc(&d.lane_do[l], o_cap));
    }
    d.lane_x_cap = x_cap;
    d.lane_o_cap = o_cap;
  }
  for (int l = 0; l < 2; ++l)
    if (!d.lane_stream[l]) TI_HIP(hipStreamCreateWithFlags(&d.lane_stream[l], hipStreamNonBlocking));
  const int64_t n_chunks = (rows + ch - 1) / ch;
  int64_t pending[2] = {-1, -1};   // chunk whose result lane l still holds
  auto drain = [&](int l) -> int {
    if (pending[l] < 0) return TI_OK;
    TI_HIP(hipStreamSynchronize(d.lane_stream[l]));
    const int64_t c = pending[l];
    const int64_t n = std::min(ch, rows - c * ch);
    copy_parallel(out + static_cast<size_t>(c * ch) * os, d.lane_ho[l], static_cast<size_t>(n) * os);
    pending[l] = -1;
    return TI_OK;
  };
  int rc = TI_OK;
  for (int64_t c = 0; c < n_chunks && rc == TI_OK; ++c) {
    const int l = static_cast<int>(c & 1);
    if ((rc = drain(l))) break;
    const int64_t r0 = c * ch;
    const int64_t n = std::min(ch, rows - r0);
    const size_t xb = static_cast<size_t>((n - 1) * stride + cols) * xs;
    copy_parallel(d.lane_hx[l], X + static_cast<size_t>(r0) * x_row, xb);
    hipStream_t st = d.lane_stream[l];
    TI_HIP(hipMemcpyAsync(d.lane_dx[l], d.lane_hx[l], xb, hipMemcpyHostToDevice, st));
    if ((rc = launch_any(f, slot, d.lane_dx[l], xdt, n, cols, stride, kind, d.lane_do[l], st)))
      break;
    TI_HIP(hipMemcpyAsync(d.lane_ho[l], d.lane_do[l], static_cast<size_t>(n) * os,
                          hipMemcpyDeviceToHost, st));
    pending[l] = c;
  }
  // the other lane first: it holds the older chunk
  const int last = static_cast<int>((n_chunks - 1) & 1);
  const int r1 = drain(last ^ 1);
  const int r2 = drain(last);
  return rc ? rc : (r1 ? r1 : r2);
}

// A caller's host span page-locked for one call (hipHostRegister over its
// page-rounded range) and unlocked when this goes out of scope.  Only a
// registration this call made counts: pages that another registration already
// holds (hipErrorHostMemoryAlreadyRegistered) may be unlocked by their owner
// mid-DMA, so reg() reports failure and the caller takes the staging chunks.
struct HostSpan {
  void* p = nullptr;
  bool mine = false;
  bool reg(const void* base, size_t n, bool portable = false) {
    const uintptr_t pg = 4096;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base) & ~(pg - 1);
    const uintptr_t hi = (reinterpret_cast<uintptr_t>(base) + n + pg - 1) & ~(pg - 1);
    p = reinterpret_cast<void*>(lo);
    const hipError_t e = hipHostRegister(p, hi - lo, portable ? hipHostRegisterPortable
                                                                : hipHostRegisterDefault);
    if (e == hipSuccess) {
      mine = true;
      return true;
    }
    (void)hipGetLastError();
    return false;
  }
  ~HostSpan() {
    if (mine) (void)hipHostUnregister(p);
  }
};

// The caller's own buffers page-locked for the call (hipHostRegister), so
// chunks go H2D straight from X and D2H straight into out, alternating two
// lanes with no host copy and no host wait until the end (TI_OPT_HOST_REGISTER;
// A/B against the pinned-chunk pipeline, which copies every byte once on the
// host).  Returns TI_ERR_UNSUPPORTED, having done nothing, when a buffer
// cannot be registered; the caller then takes the pinned-chunk pipeline.
// `pre`: the caller registered X and out already (the multi-device ti_predict
// registers the whole batch once, before its shard threads start).
int predict_registered(ti_forest* f, int slot, DeviceForest& d, const unsigned char* X, int xdt,
                       int64_t rows, int32_t cols, int64_t stride, int kind, unsigned char* out,
                       int64_t ch, bool pre) {
  const size_t xs = dtype_size(xdt);
  const size_t os = dtype_size(output_dtype(f, kind)) * output_width(f, kind);
  const size_t x_row = static_cast<size_t>(stride) * xs;
  const size_t x_bytes = static_cast<size_t>((rows - 1) * stride + cols) * xs;
  const size_t o_bytes = static_cast<size_t>(rows) * os;
  HostSpan rx, ro;
  if (!pre && (!rx.reg(X, x_bytes) || !ro.reg(out, o_bytes))) return TI_ERR_UNSUPPORTED;
  struct LaneSync {
    DeviceForest& d;
    ~LaneSync() {
      for (int l = 0; l < 2; ++l)
        if (d.lane_stream[l]) (void)hipStreamSynchronize(d.lane_stream[l]);
    }
  } lane_sync{d};
  const size_t x_cap = static_cast<size_t>(ch) * x_row;
  const size_t o_cap = static_cast<size_t>(ch) * os;
  if (d.lane_x_cap < x_cap || d.lane_o_cap < o_cap) {
    for (int l = 0; l < 2; ++l) {
      if (d.lane_hx[l]) (void)hipHostFree(d.lane_hx[l]);
      if (d.lane_ho[l]) (void)hipHostFree(d.lane_ho[l]);
      if (d.lane_dx[l]) (void)hipFree(d.lane_dx[l]);
      if (d.lane_do[l]) (void)hipFree(d.lane_do[l]);
      d.lane_hx[l] = d.lane_ho[l] = d.lane_dx[l] = d.lane_do[l] = nullptr;
    }
    d.lane_x_cap = d.lane_o_cap = 0;
    for (int l = 0; l < 2; ++l) {
      TI_HIP(hipHostMalloc(&d.lane_hx[l], x_cap, hipHostMallocDefault));
      TI_HIP(hipHostMalloc(&d.lane_ho[l], o_cap, hipHostMallocDefault));
      TI_HIP(hipMalloc(&d.lane_dx[l], x_cap));
      TI_HIP(hipMalloc(&d.lane_do[l], o_cap));
    }
    d.lane_x_cap = x_cap;
    d.lane_o_cap = o_cap;
  }
  for (int l = 0; l < 2; ++l)
    if (!d.lane_stream[l]) TI_HIP(hipStreamCreateWithFlags(&d.lane_stream[l], hipStreamNonBlocking));
  const int64_t n_chunks = (rows + ch - 1) / ch;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const int l = static_cast<int>(c & 1);
    const int64_t r0 = c * ch;
    const int64_t n = std::min(ch, rows - r0);
    const size_t xb = static_cast<size_t>((n - 1) * stride + cols) * xs;
    hipStream_t st = d.lane_stream[l];
    TI_HIP(hipMemcpyAsync(d.lane_dx[l], X + static_cast<size_t>(r0) * x_row, xb,
                          hipMemcpyHostToDevice, st));
    int rc = launch_any(f, slot, d.lane_dx[l], xdt, n, cols, stride, kind, d.lane_do[l], st);
    if (rc) return rc;
    TI_HIP(hipMemcpyAsync(out + static_cast<size_t>(r0) * os, d.lane_do[l], static_cast<size_t>(n) * os,
                          hipMemcpyDeviceToHost, st));
  }
  for (int l = 0; l < 2; ++l) TI_HIP(hipStreamSynchronize(d.lane_stream[l]));
  return TI_OK;
}

// reg: 0 pinned staging chunks; 1 page-lock this shard's X and out for the
// call (one device); 2 the caller page-locked the whole batch (multi-device)
int predict_shard(ti_forest* f, int slot, DeviceForest& d, const unsigned char* X, int xdt,
                  int64_t rows, int32_t cols, int64_t stride, int kind, unsigned char* out,
                  int reg) {
  std::lock_guard<std::mutex> lk(d.mu);
  TI_HIP(hipSetDevice(d.device));
  {
    const int64_t ch = chunk_rows_for(f, xdt, stride, kind);
    if (rows > ch) {
      if (reg) {
        const int rc = predict_registered(f, slot, d, X, xdt, rows, cols, stride, kind, out, ch,
                                          reg == 2);
        if (rc != TI_ERR_UNSUPPORTED) return rc;
      }
      return predict_pipelined(f, slot, d, X, xdt, rows, cols, stride, kind, out, ch);
    }
  }
  const size_t xs = dtype_size(xdt);
  const size_t x_elems = static_cast<size_t>((rows - 1) * stride + cols);
  const size_t out_bytes = static_cast<size_t>(rows * output_width(f, kind)) *
                           dtype_size(output_dtype(f, kind));
  int rc;
  const size_t x_bytes = x_elems * xs;
  if ((rc = grow(&d.x_buf, &d.x_cap, x_bytes))) return rc;
  if ((rc = grow(&d.out_buf, &d.out_cap, out_bytes))) return rc;
  if ((rc = grow(&d.hx_pin, &d.hx_cap, x_bytes, true))) return rc;
  if ((rc = grow(&d.ho_pin, &d.ho_cap, out_bytes, true))) return rc;
  // caller memory -> pinned staging -> DMA; keeps H2D/D2H asynchronous and at
  // PCIe rate whatever kind of host memory the caller holds
  copy_parallel(d.hx_pin, X, x_bytes);
  TI_HIP(hipMemcpyAsync(d.x_buf, d.hx_pin, x_bytes, hipMemcpyHostToDevice, d.stream));
  if ((rc = launch_any(f, slot, d.x_buf, xdt, rows, cols, stride, kind, d.out_buf, d.stream)))
    return rc;
  TI_HIP(hipMemcpyAsync(d.ho_pin, d.out_buf, out_bytes, hipMemcpyDeviceToHost, d.stream));
  TI_HIP(hipStreamSynchronize(d.stream));
  copy_parallel(out, d.ho_pin, out_bytes);
  return TI_OK;
}

// ------------------------------------------------- more than 16 output groups
// Output transform over [rows, K] margins for forests split into group parts
// (the fused epilogue covers K <= kMaxGroups).  Same arithmetic as
// ti::finish_row: softmax with the maximum in ACC and the sum in double,
// first-maximum argmax.
template <typename ACC>
__global__ void transform_rows_kernel(const ACC* __restrict__ m, int64_t rows, int K, int tr,
                                      double param, ACC* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const ACC* v = m + r * K;
  if (tr == TI_TRANSFORM_ARGMAX) {
    int best = 0;
    for (int k = 1; k < K; ++k)
      if (v[best] < v[k]) best = k;
    out[r] = (ACC)best;
    return;
  }
  ACC* o = out + r * K;
  if (tr == TI_TRANSFORM_SOFTMAX) {
    ACC wmax = v[0];
    for (int k = 1; k < K; ++k) wmax = (v[k] < wmax) ? wmax : v[k];
    double wsum = 0.0;
    for (int k = 0; k < K; ++k) wsum += ti::t_exp(v[k] - wmax);
    for (int k = 0; k < K; ++k) o[k] = ti::t_exp(v[k] - wmax) / (ACC)wsum;
    return;
  }
  for (int k = 0; k < K; ++k) {
    ACC x = v[k];
    switch (tr) {
      case TI_TRANSFORM_SIGMOID: x = ACC(1) / (ACC(1) + ti::t_exp(-((ACC)param * x))); break;
      case TI_TRANSFORM_HINGE: x = x > ACC(0) ? ACC(1) : ACC(0); break;
      case TI_TRANSFORM_EXP: x = ti::t_exp(x); break;
      case TI_TRANSFORM_SIGNSQUARE: x = (ACC)((x > ACC(0)) - (x < ACC(0))) * x * x; break;
      case TI_TRANSFORM_LOG1PEXP: x = ti::t_log1p(ti::t_exp(x)); break;
      case TI_TRANSFORM_STEP: x = x >= ACC(0) ? ACC(1) : ACC(0); break;
      default: break;
    }
    o[k] = x;
  }
}

// dst[r, map[j]] = src[r, j] for the leaf-id columns of one part.
__global__ void scatter_cols_kernel(const int32_t* __restrict__ src, int64_t rows, int tc,
                                    const int32_t* __restrict__ map, int T,
                                    int32_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * tc) return;
  const int64_t r = i / tc;
  const int j = (int)(i - r * tc);
  dst[r * T + map[j]] = src[i];
}

// Device path of a chunked forest: each part writes its margin columns (or
// leaf-id columns) through a scratch buffer of the replica's (CallScratch),
// then the output transform runs over the assembled [rows, K] margins.
int launch_chunked(ti_forest* f, int slot, const void* X, int xdt, int64_t rows, int32_t cols,
                   int64_t stride, int kind, void* out, hipStream_t stream) {
  const size_t as = f->accum == TI_F64 ? 8 : 4;
  const int threads = 256;
  if (kind == TI_OUTPUT_LEAF && f->LW != 1)   // vector leaves: every part holds every tree
    return launch_any(f->parts[0].get(), slot, X, xdt, rows, cols, stride, kind, out, stream);
  int rc = TI_OK;
  size_t tmp_bytes = 0;
  if (kind == TI_OUTPUT_INTERACT) {
    // (F + 1)^2 columns a group.  A part's finishing kernel writes its groups'
    // matrices straight into their columns of the [rows, K, F + 1, F + 1]
    // output (row pitch = the whole forest's row): the largest output there is
    // gets no scratch copy and no second pass over it.
    const int64_t cw = static_cast<int64_t>(f->F + 1) * (f->F + 1);
    for (size_t c = 0; c < f->parts.size(); ++c) {
      ti_forest* p = f->parts[c].get();
      const int rc = launch_interact(p, *p->devs[slot], X, xdt, rows, cols, stride,
                                     static_cast<unsigned char*>(out) + f->part_k0[c] * cw * as,
                                     f->K * cw, stream);
      if (rc) return rc;
    }
    return TI_OK;
  }
  if (kind == TI_OUTPUT_CONTRIB_APPROX) {
    // F + 1 columns a group, written by each part's pass 2 straight into its
    // groups' columns of the [rows, K * (F + 1)] output, as above: not through
    // the shared scratch and 2-D copy of TI_OUTPUT_CONTRIB below.  Vector-leaf
    // parts hold every tree and walk it once each.
    const int64_t cw = f->F + 1;
    for (size_t c = 0; c < f->parts.size(); ++c) {
      ti_forest* p = f->parts[c].get();
      const int rc = launch_approx(p, *p->devs[slot], X, xdt, rows, cols, stride,
                                   static_cast<unsigned char*>(out) + f->part_k0[c] * cw * as,
                                   f->K * cw, stream);
      if (rc) return rc;
    }
    return TI_OK;
  }
  const int64_t cw = kind == TI_OUTPUT_CONTRIB ? f->F + 1 : 1;   // columns per group
  for (auto& p : f->parts)
    tmp_bytes = std::max(tmp_bytes, static_cast<size_t>(rows) *
                                        (kind == TI_OUTPUT_LEAF ? 4 * p->T : as * p->K * cw));
  // the replica that serves the slot: the first part's (base_forest)
  DeviceForest& sd = *f->parts[0]->devs[slot];
  ScratchHold tmp_buf(sd, stream), marg_buf(sd, stream);   // given back behind the last kernel below
  if (!tmp_buf.take(tmp_bytes)) return fail(TI_ERR_NOMEM, "part scratch allocation failed");
  void* tmp = tmp_buf.p;
  const bool transform = kind == TI_OUTPUT_PREDICT && f->transform != TI_TRANSFORM_IDENTITY;
  if (transform && !marg_buf.take(static_cast<size_t>(rows) * f->K * as))
    return fail(TI_ERR_NOMEM, "margin scratch allocation failed");
  void* marg = marg_buf.p;
  void* mdst = transform ? marg : out;
  for (size_t c = 0; c < f->parts.size() && rc == TI_OK; ++c) {
    ti_forest* p = f->parts[c].get();
    if (kind == TI_OUTPUT_LEAF) {
      rc = launch_any(p, slot, X, xdt, rows, cols, stride, kind, tmp, stream);
      if (rc) break;
      const std::vector<int32_t>& map = f->part_trees[c];
      ScratchHold map_buf(sd, stream);   // given back behind scatter_cols_kernel
      int32_t* dmap = map_buf.take(map.size() * 4) ? static_cast<int32_t*>(map_buf.p) : nullptr;
      if (!dmap || hipMemcpyAsync(dmap, map.data(), map.size() * 4, hipMemcpyHostToDevice, stream) !=
                       hipSuccess) {
        rc = fail(TI_ERR_DEVICE, "leaf map upload failed");
        break;
      }
      const int64_t n = rows * p->T;
      hipLaunchKernelGGL(scatter_cols_kernel, dim3(static_cast<unsigned>((n + threads - 1) / threads)),
                         dim3(threads), 0, stream, static_cast<const int32_t*>(tmp), rows, p->T,
                         dmap, f->T, static_cast<int32_t*>(out));
    } else {
      const int pk = kind == TI_OUTPUT_CONTRIB ? TI_OUTPUT_CONTRIB : TI_OUTPUT_MARGIN;
      rc = launch_any(p, slot, X, xdt, rows, cols, stride, pk, tmp, stream);
      if (rc) break;
      if (hipMemcpy2DAsync(static_cast<unsigned char*>(mdst) + f->part_k0[c] * cw * as,
                           f->K * cw * as, tmp, p->K * cw * as, p->K * cw * as, rows,
                           hipMemcpyDeviceToDevice, stream) != hipSuccess)
        rc = fail(TI_ERR_DEVICE, "margin column copy failed");
    }
  }
  if (rc == TI_OK && transform) {
    const unsigned grid = static_cast<unsigned>((rows + threads - 1) / threads);
    if (f->accum == TI_F64)
      hipLaunchKernelGGL(transform_rows_kernel<double>, dim3(grid), dim3(threads), 0, stream,
                         static_cast<const double*>(marg), rows, f->K, f->transform, f->tparam,
                         static_cast<double*>(out));
    else
      hipLaunchKernelGGL(transform_rows_kernel<float>, dim3(grid), dim3(threads), 0, stream,
                         static_cast<const float*>(marg), rows, f->K, f->transform, f->tparam,
                         static_cast<float*>(out));
    if (hipGetLastError() != hipSuccess) rc = fail(TI_ERR_DEVICE, "transform launch failed");
  }
  return rc;
}

// Linear leaves: two stream-ordered passes per row block.  Pass 1 is the
// forest's own walk with TI_OUTPUT_LEAF into a [rows_block, T] int32 scratch;
// pass 2 (linear_leaf_kernel) evaluates each reached leaf's linear model on
// the raw features and finishes the row.  A block is as many whole tiles of
// pass 2 as fit TI_OPT_LINEAR_SCRATCH_MB, at least one.
int launch_linear(ti_forest* f, DeviceForest& d, const void* X, int xdt, int64_t rows, int32_t cols,
                  int64_t stride, int kind, void* out, hipStream_t stream) {
  if (rows <= 0) return TI_OK;
  const size_t xs = dtype_size(xdt);
  // TI_LINEAR_FEAT_LDS=0 (developer knob): features from HBM even where the image fits (an A/B)
  const int R = env_int("TI_LINEAR_FEAT_LDS", 1) != 0 ? pick_rows(f->F, xs, 0) : 0;   // 0: HBM
  const bool feat_lds = R > 0;
  const int block = feat_lds ? R : 256;
  const size_t lds = (feat_lds ? align16(static_cast<size_t>(f->F) * block * xs) : 0) + 16 +
                     static_cast<size_t>(block) * ti::kLinPitch * 4;
  LaunchPlan p;   // the shared prologue's and epilogue's arguments, as every walk gets them
  int rc = plan_launch(f, d, xdt, kind, &p);
  if (rc) return rc;
  ti::LinearFn fn = xdt == TI_F64 ? ti::select_linear<double>(f->K, feat_lds)
                                  : ti::select_linear<float>(f->K, feat_lds);
  rc = ensure_lds_attr(d.device, reinterpret_cast<KernelFn>(fn));
  if (rc) return rc;
  const int64_t row_bytes = static_cast<int64_t>(4) * f->T;
  int64_t rows_block = (f->lin_scratch_mb.load() << 20) / row_bytes;
  rows_block = std::max<int64_t>(block, rows_block / block * block);
  rows_block = std::min(rows_block, (rows + block - 1) / block * block);
  ScratchHold ids_buf(d, stream);   // given back behind the last pass 2
  if (!ids_buf.take(static_cast<size_t>(std::min(rows, rows_block) * row_bytes)))
    return fail(TI_ERR_NOMEM, "leaf-id scratch allocation failed");
  int32_t* ids = static_cast<int32_t*>(ids_buf.p);
  const size_t out_row = static_cast<size_t>(output_width(f, kind)) * 8;
  for (int64_t r0 = 0; r0 < rows && rc == TI_OK; r0 += rows_block) {
    const int64_t nb = std::min(rows_block, rows - r0);
    const void* xb = static_cast<const unsigned char*>(X) + static_cast<size_t>(r0 * stride) * xs;
    rc = launch(f, d, xb, xdt, nb, cols, stride, TI_OUTPUT_LEAF, ids, stream);
    if (rc) break;
    KArgs a = p.a;
    a.X = xb;
    a.n_rows = nb;
    a.row_stride = stride;
    a.n_cols = cols;
    a.out = static_cast<unsigned char*>(out) + static_cast<size_t>(r0) * out_row;
    ti::LinArgs la;
    la.leaf_ids = ids;
    la.leaves = d.lin_leaves;
    la.terms = d.lin_terms;
    la.leaf_base = d.lin_leaf_base;
    hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>((nb + block - 1) / block)), dim3(block), lds,
                       stream, a, la);
    if (hipGetLastError() != hipSuccess) rc = fail(TI_ERR_DEVICE, "linear leaf launch failed");
  }
  return rc;
}

// Approximate contributions (treeinfer_approx.h): two stream-ordered passes per
// row block.  Pass 1 is the forest's own walk with TI_OUTPUT_LEAF into a
// [rows_block, T] int32 scratch, bounded as launch_linear bounds its own (1 GiB;
// TI_APPROX_SCRATCH_MB is the developer knob, 0: one tile a block); pass 2
// (approx_contrib_kernel) adds the reached leaves' terms and writes the rows
// through out_ld, the elements between two output rows.
constexpr int64_t kApproxWorkgroupTarget = 1536;        // 256 CUs x 6 workgroups (C2's LDS)
constexpr int kApproxMaxSlices = 32;
constexpr uint64_t kApproxPartBytesMax = 64ull << 20;   // the slices' partials of one row block

int launch_approx(ti_forest* f, DeviceForest& d, const void* X, int xdt, int64_t rows, int32_t cols,
                  int64_t stride, void* out, int64_t out_ld, hipStream_t stream) {
  if (f->approx_refused)
    return fail(TI_ERR_UNSUPPORTED,
                f->approx_refused == 2
                    ? "TI_OUTPUT_CONTRIB_APPROX of a forest with linear leaves (a leaf has no one "
                      "value to take node means of)"
                    : "approximate contributions need node covers (ti_forest_desc.cover)");
  if (rows <= 0) return TI_OK;
  int rc = ensure_approx(f);
  if (rc) return rc;
  constexpr int R = ti::kApproxRows;
  const int64_t W = static_cast<int64_t>(f->K) * (f->F + 1);
  const int n_tiles = static_cast<int>((W + ti::kApproxCols - 1) / ti::kApproxCols);
  const int col_tile = static_cast<int>((W + n_tiles - 1) / n_tiles);
  const size_t lds = static_cast<size_t>(col_tile) * ti::kApproxPitch * 8 +
                     static_cast<size_t>(R) * ti::kLinPitch * 4;
  using ApproxFn = void (*)(ti::ApproxArgs);
  const ApproxFn fn = f->accum == TI_F64 ? ti::approx_contrib_kernel<double, double>
                                         : ti::approx_contrib_kernel<float, float>;
  rc = ensure_lds_attr(d.device, reinterpret_cast<KernelFn>(fn));
  if (rc) return rc;
  occ_note(reinterpret_cast<KernelFn>(fn), R, lds);
  const size_t xs = dtype_size(xdt), as = dtype_size(f->accum);
  const int64_t row_bytes = static_cast<int64_t>(4) * f->T;
  int64_t rows_block = (static_cast<int64_t>(std::max(env_int("TI_APPROX_SCRATCH_MB", 1024), 0)) << 20) / row_bytes;
  rows_block = std::max<int64_t>(R, rows_block / R * R);
  const int64_t rows_max = std::min(rows, rows_block);
  // Tree slices: a block of few rows is too few single-wave workgroups for 256
  // CUs with six of them each, so its trees are cut into slices of whole
  // 32-tree id chunks until about that many workgroups run; the slices' raw
  // float64 sums [slices][rows][W] (at most 64 MiB, else fewer slices) are
  // added in slice order by approx_slices_kernel.  TI_APPROX_SLICES (developer
  // knob) forces the count (1: none).
  const int64_t n_chunks = (f->T + ti::kLinTC - 1) / ti::kLinTC;
  const int64_t wgs = (rows_max + R - 1) / R * n_tiles;
  const int force_slices = env_int("TI_APPROX_SLICES", 0);
  int64_t want = force_slices > 0 ? force_slices : kApproxWorkgroupTarget / wgs;
  while (want > 1 && static_cast<uint64_t>(want) * rows_max * W * 8 > kApproxPartBytesMax) --want;
  want = std::max<int64_t>(1, std::min({want, n_chunks, int64_t(kApproxMaxSlices)}));
  const int32_t slice_chunks = static_cast<int32_t>((n_chunks + want - 1) / want);
  const int slices = static_cast<int>((n_chunks + slice_chunks - 1) / slice_chunks);
  ScratchHold ids_buf(d, stream), part_buf(d, stream);   // given back behind the last pass 2
  if (!ids_buf.take(static_cast<size_t>(rows_max * row_bytes)))
    return fail(TI_ERR_NOMEM, "leaf-id scratch allocation failed");
  int32_t* ids = static_cast<int32_t*>(ids_buf.p);
  if (slices > 1 && !part_buf.take(static_cast<size_t>(slices * rows_max * W) * 8))
    return fail(TI_ERR_NOMEM, "slice partials allocation failed");
  double* part = static_cast<double*>(part_buf.p);
  for (int64_t r0 = 0; r0 < rows && rc == TI_OK; r0 += rows_block) {
    const int64_t nb = std::min(rows_block, rows - r0);
    const void* xb = static_cast<const unsigned char*>(X) + static_cast<size_t>(r0 * stride) * xs;
    rc = launch(f, d, xb, xdt, nb, cols, stride, TI_OUTPUT_LEAF, ids, stream);
    if (rc) break;
    ti::ApproxArgs a;
    a.leaf_ids = ids;
    a.leaves = d.approx_leaves;
    a.terms = d.approx_terms;
    a.leaf_base = d.approx_leaf_base;
    a.bias = d.approx_bias;
    a.n_rows = nb;
    a.n_trees = f->T;
    a.width = static_cast<int32_t>(W);
    a.f1 = f->F + 1;
    a.col_tile = col_tile;
    a.n_col_tiles = n_tiles;
    a.divisor = f->divisor;
    a.out = static_cast<unsigned char*>(out) + static_cast<size_t>(r0 * out_ld) * as;
    a.out_ld = out_ld;
    a.slice_chunks = slice_chunks;
    a.part = part;
    const int64_t grid = (nb + R - 1) / R;
    if (grid > 0x7fffffff) rc = fail(TI_ERR_INVALID, "too many rows for one launch");
    if (rc) break;
    hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(grid), static_cast<unsigned>(std::min(n_tiles, 65535)),
                                static_cast<unsigned>(slices)),
                       dim3(R), lds, stream, a);
    if (slices > 1) {
      const int64_t n = nb * W;
      if (f->accum == TI_F64)
        hipLaunchKernelGGL(ti::approx_slices_kernel<double>, dim3(static_cast<unsigned>((n + 255) / 256)),
                           dim3(256), 0, stream, a, slices);
      else
        hipLaunchKernelGGL(ti::approx_slices_kernel<float>, dim3(static_cast<unsigned>((n + 255) / 256)),
                           dim3(256), 0, stream, a, slices);
    }
    if (hipGetLastError() != hipSuccess) rc = fail(TI_ERR_DEVICE, "approximate contributions launch failed");
  }
  return rc;
}

// The forest's walk of X as it stands: every kind, every forest shape.
int launch_walk(ti_forest* f, int slot, const void* X, int xdt, int64_t rows, int32_t cols,
                int64_t stride, int kind, void* out, hipStream_t stream) {
  if (kind == TI_OUTPUT_CONTRIB_APPROX && f->parts.empty())
    return launch_approx(f, *f->devs[slot], X, xdt, rows, cols, stride, out, output_width(f, kind),
                         stream);
  if (kind == TI_OUTPUT_CONTRIB && f->linear)
    return fail(TI_ERR_UNSUPPORTED,
                "TI_OUTPUT_CONTRIB of a forest with linear leaves (LightGBM itself refuses "
                "pred_contrib on a linear-tree model)");
  if (kind == TI_OUTPUT_INTERACT && f->linear)
    return fail(TI_ERR_UNSUPPORTED,
                "TI_OUTPUT_INTERACT of a forest with linear leaves (contributions of a linear-tree "
                "model are refused too)");
  if (kind == TI_OUTPUT_CONTRIB && f->parts.empty())
    return launch_contrib(f, *f->devs[slot], X, xdt, rows, cols, stride, out, stream);
  if (kind == TI_OUTPUT_INTERACT && f->parts.empty())
    return launch_interact(f, *f->devs[slot], X, xdt, rows, cols, stride, out,
                           output_width(f, kind), stream);
  if (!f->parts.empty())
    return launch_chunked(f, slot, X, xdt, rows, cols, stride, kind, out, stream);
  if (f->linear && (kind == TI_OUTPUT_MARGIN || kind == TI_OUTPUT_PREDICT))
    return launch_linear(f, *f->devs[slot], X, xdt, rows, cols, stride, kind, out, stream);
  return launch(f, *f->devs[slot], X, xdt, rows, cols, stride, kind, out, stream);
}

ti_forest* base_forest(ti_forest* f);

// pre_steps_kernel over a batch: S steps with the arrays of replica d (S = 0:
// the plain conversion to float32), dense float32 [rows, cols] into `out`.
int launch_pre_steps(const DeviceForest& d, int S, const void* X, int xdt, int64_t rows,
                     int32_t cols, int64_t stride, float* out, hipStream_t stream) {
  if (rows <= 0) return TI_OK;
  ti::PreArgs a;
  a.X = X;
  a.out = out;
  a.ops = d.pre_op;
  a.consts = d.pre_const;
  a.row_stride = stride;
  a.total = static_cast<uint64_t>(rows) * static_cast<uint64_t>(cols);
  a.n_cols = static_cast<uint32_t>(cols);
  a.n_steps = S;
  const uint64_t per_wg = static_cast<uint64_t>(ti::kPreBlock) * ti::kPreUnroll;
  const uint32_t grid = static_cast<uint32_t>(
      std::min<uint64_t>((a.total + per_wg - 1) / per_wg, ti::kPreMaxGrid));
  a.step = grid * ti::kPreBlock;
  a.step_rows = a.step / a.n_cols;
  a.step_cols = a.step % a.n_cols;
  const size_t const_bytes = static_cast<size_t>(S) * cols * 8;
  const bool lds = const_bytes <= ti::kPreLdsBudget;
  const size_t lds_bytes = lds ? align16(const_bytes + static_cast<size_t>(S) * 4) : 0;
  hipLaunchKernelGGL(ti::select_pre(xdt == TI_F64, lds), dim3(grid), dim3(ti::kPreBlock), lds_bytes,
                     stream, a);
  TI_HIP(hipGetLastError());
  return TI_OK;
}

// Where X enters.  A forest with pre-steps transforms the batch once into a
// float32 scratch of the slot's replica (given back behind the walk's last
// kernel) and walks that; its group parts (launch_chunked) and every
// two-pass kind then read the transformed rows.  A forest without pre-steps
// goes straight to its walk.
int launch_any(ti_forest* f, int slot, const void* X, int xdt, int64_t rows, int32_t cols,
               int64_t stride, int kind, void* out, hipStream_t stream) {
  if (f->pre_steps <= 0 || rows <= 0)
    return launch_walk(f, slot, X, xdt, rows, cols, stride, kind, out, stream);
  if (cols != f->F)
    return fail(TI_ERR_INVALID, "a forest with pre-steps needs n_cols == n_features (" +
                                    std::to_string(f->F) + "), got " + std::to_string(cols));
  DeviceForest& d = *base_forest(f)->devs[slot];
  ScratchHold xt(d, stream);
  if (!xt.take(static_cast<size_t>(rows) * cols * 4))
    return fail(TI_ERR_NOMEM, "pre-step scratch allocation failed");
  const int rc = launch_pre_steps(d, f->pre_steps, X, xdt, rows, cols, stride,
                                  static_cast<float*>(xt.p), stream);
  if (rc) return rc;
  return launch_walk(f, slot, xt.p, TI_F32, rows, cols, cols, kind, out, stream);
}

// Split a forest of K > kMaxGroups outputs into parts of at most kMaxGroups
// groups.  Scalar leaves (leaf_width 1, XGBoost / LightGBM multiclass): a
// part holds the trees of its groups, in their original order, so each
// group's sum is bit-identical.  Vector leaves (sklearn classifiers): every
// part holds every tree with its slice of the leaf vectors.
int create_chunked(const ti_forest_desc* d, const std::vector<int>& depth, const int32_t* devices,
                   int32_t n_devices, ti_forest** out) {
  std::unique_ptr<ti_forest> f(new ti_forest());
  fill_model(d, depth, f.get());
  f->lgb_zero_map = 0;   // the parts hold it: a parent launches no tree kernel
  const int K = d->n_groups, LW = d->leaf_width;
  for (int k0 = 0; k0 < K; k0 += ti::kMaxGroups) {
    const int kc = std::min(ti::kMaxGroups, K - k0);
    std::vector<int32_t> trees, tgrp, feat, left, right, leaf_id, cat_nw;
    std::vector<int64_t> toff(1, 0), cat_off;
    std::vector<double> thr, lv, cov, base(d->base_margin + k0, d->base_margin + k0 + kc);
    std::vector<uint8_t> flags;
    for (int t = 0; t < d->n_trees; ++t) {
      if (LW == 1 && (d->tree_group[t] < k0 || d->tree_group[t] >= k0 + kc)) continue;
      trees.push_back(t);
      tgrp.push_back(LW == 1 ? d->tree_group[t] - k0 : 0);
      for (int64_t g = d->tree_offset[t]; g < d->tree_offset[t + 1]; ++g) {
        feat.push_back(d->feature[g]);
        thr.push_back(d->threshold[g]);
        flags.push_back(d->flags[g]);
        left.push_back(d->left[g]);
        right.push_back(d->right[g]);
        leaf_id.push_back(d->leaf_id[g]);
        if (d->cover) cov.push_back(d->cover[g]);
        if (d->cat_offset) {
          cat_off.push_back(d->cat_offset[g]);
          cat_nw.push_back(d->cat_nwords[g]);
        }
        if (LW == 1) {
          lv.push_back(d->leaf_value[g]);
        } else {
          for (int k = 0; k < kc; ++k) lv.push_back(d->leaf_value[g * LW + k0 + k]);
        }
      }
      toff.push_back(static_cast<int64_t>(feat.size()));
    }
    if (trees.empty())
      return fail(TI_ERR_UNSUPPORTED, "output groups " + std::to_string(k0) + ".." +
                                          std::to_string(k0 + kc - 1) + " have no trees");
    ti_forest_desc sd = *d;
    sd.n_trees = static_cast<int32_t>(trees.size());
    sd.n_groups = kc;
    sd.leaf_width = LW == 1 ? 1 : kc;
    sd.n_nodes = static_cast<int64_t>(feat.size());
    sd.tree_offset = toff.data();
    sd.tree_group = tgrp.data();
    sd.feature = feat.data();
    sd.threshold = thr.data();
    sd.flags = flags.data();
    sd.left = left.data();
    sd.right = right.data();
    sd.leaf_id = leaf_id.data();
    sd.leaf_value = lv.data();
    sd.base_margin = base.data();
    sd.transform = TI_TRANSFORM_IDENTITY;
    sd.transform_param = 1.0;
    sd.cat_offset = d->cat_offset ? cat_off.data() : nullptr;
    sd.cat_nwords = d->cat_offset ? cat_nw.data() : nullptr;
    sd.cover = d->cover ? cov.data() : nullptr;
    if (k0 > 0) {   // the first part's replicas hold the pre-step arrays
      sd.n_pre_steps = 0;
      sd.pre_op = nullptr;
      sd.pre_const = nullptr;
    }
    ti_forest* part = nullptr;
    const int rc = ti_forest_create(&sd, devices, n_devices, &part);
    if (rc) {
      for (auto& q : f->parts) ti_forest_destroy(q.release());
      return rc;
    }
    part->pre_steps = 0;   // the parent transforms X once (launch_any); no part does
    f->parts.emplace_back(part);
    f->part_k0.push_back(k0);
    f->part_trees.push_back(std::move(trees));
  }
  f->layout = f->parts[0]->layout;
  *out = f.release();
  return TI_OK;
}

// The forest whose DeviceForest (stream, staging buffers, lock) serves a slot.
ti_forest* base_forest(ti_forest* f) {   // declared above launch_any
  while (!f->parts.empty()) f = f->parts[0].get();
  return f;
}

}  // namespace

extern "C" {

int32_t ti_abi_version(void) { return TI_ABI_VERSION; }

const char* ti_last_error(void) { return g_last_error.c_str(); }

int ti_device_count(int32_t* count) {
  if (!count) return fail(TI_ERR_INVALID, "null count");
  int n = 0;
  TI_HIP(hipGetDeviceCount(&n));
  *count = n;
  return TI_OK;
}

int ti_forest_create(const ti_forest_desc* desc, const int32_t* devices, int32_t n_devices,
                     ti_forest** out) {
  if (!out) return fail(TI_ERR_INVALID, "null output handle");
  *out = nullptr;
  if (!devices || n_devices <= 0) return fail(TI_ERR_INVALID, "need at least one device");
  std::vector<int> depth;
  int rc = validate(desc, &depth);
  if (rc) return rc;
  int n_visible = 0;
  TI_HIP(hipGetDeviceCount(&n_visible));
  for (int i = 0; i < n_devices; ++i)
    if (devices[i] < 0 || devices[i] >= n_visible)
      return fail(TI_ERR_INVALID, "device ordinal " + std::to_string(devices[i]) + " not visible");
  if (desc->n_groups > ti::kMaxGroups) return create_chunked(desc, depth, devices, n_devices, out);

  std::unique_ptr<ti_forest> f(new ti_forest());
  fill_model(desc, depth, f.get());
  f->host = std::make_unique<HostImage>();
  if ((rc = choose_layout(desc, f.get()))) return rc;
  if (desc->lin_offset && (rc = pack_linear(desc, f->host.get()))) return rc;
  keep_shap_source(desc, f.get());
  keep_approx_source(desc, f.get());
  if (desc->n_pre_steps > 0) {
    f->host->pre_op.assign(desc->pre_op, desc->pre_op + desc->n_pre_steps);
    f->host->pre_const.assign(desc->pre_const,
                              desc->pre_const + static_cast<size_t>(desc->n_pre_steps) * desc->n_features);
  }
  for (int i = 0; i < n_devices; ++i) {
    f->devs.emplace_back(new DeviceForest());
    rc = upload_device(f.get(), *f->devs.back(), devices[i]);
    if (rc) {
      for (auto& d : f->devs) free_device(*d);
      return rc;
    }
  }
  f->host.reset();   // every replica is resident (an early return drops it with the forest)
  *out = f.release();
  return TI_OK;
}

int ti_forest_destroy(ti_forest* forest) {
  if (!forest) return TI_OK;
  for (auto& p : forest->parts) ti_forest_destroy(p.release());
  for (auto& d : forest->devs) free_device(*d);
  delete forest;
  return TI_OK;
}

int ti_forest_get_info(const ti_forest* f, ti_forest_info* info) {
  if (!f || !info) return fail(TI_ERR_INVALID, "null argument");
  info->layout = f->layout;
  info->depth = f->depth;
  info->n_trees = f->T;
  info->n_groups = f->K;
  info->n_features = f->F;
  const ti_forest* bf = f;
  while (!bf->parts.empty()) bf = bf->parts[0].get();
  info->n_devices = static_cast<int32_t>(bf->devs.size());
  info->device_bytes = 0;
  if (f->parts.empty()) {
    info->device_bytes = f->devs.empty() ? 0 : f->devs[0]->bytes;
  } else {
    for (auto& p : f->parts) info->device_bytes += p->devs.empty() ? 0 : p->devs[0]->bytes;
  }
  const ti_forest* pf = f->parts.empty() ? f : f->parts[0].get();   // a chunked forest: its first part
  info->tree_stride_bytes = f->layout == kLayoutHeap ? f->stride32
                            : f->layout == kLayoutBinHeap ? f->bh[0].stride
                            : f->layout == kLayoutCatHeap ? pf->stride32 : 0;
  // walk id: the kernel variant a PMC pass was taken on (bench.py matches it)
  info->walk = bheap_fixed(f, TI_F32, TI_OUTPUT_PREDICT) ? 2 : 0;
  info->bin_bits = f->layout == kLayoutBinHeap ? (f->bh[0].b16 ? 16 : 8)
                   : is_record(f->layout) ? (f->rx[0].b8 ? 8 : 16) : 0;
  info->tree_ilp = f->layout == kLayoutRecord ? f->rx_ilp : f->layout == kLayoutHeapTop ? f->hx_ilp
                   : stages_trees(f->layout) ? f->lx_ilp : 0;
  info->n_stages = stages_trees(f->layout) ? f->n_stages : 0;
  if (f->layout == kLayoutCatHeap) {   // the stages of a float32 batch, as plan_launch sizes them
    const int64_t S = heap_stage_trees(pf, TI_F32);
    info->n_stages = S > 0 ? static_cast<int32_t>((pf->T + S - 1) / S) : 0;
  }
  info->top_depth = has_heap_top(f->layout) ? f->hx_top : 0;
  info->bottom = f->layout == kLayoutTopStaged ? f->tx8 : 0;
  // the TreeSHAP coefficient table of slot 0 (of the first part)
  const ti_forest* sf = f->parts.empty() ? f : f->parts[0].get();
  info->shap_table = sf->devs.empty() ? 0 : sf->devs[0]->shap_tab_state.load();
  info->linear = f->linear;
  info->shap_table_bytes = info->shap_table == 1 ? sf->shap_tab_len * sf->shap_tab_mt : 0;
  info->shap_table_build_ms = sf->shap_tab_build_ms;
  info->pre_steps = f->pre_steps;
  return TI_OK;
}

int ti_forest_set_option(ti_forest* f, int32_t option, int64_t value) {
  if (!f) return fail(TI_ERR_INVALID, "null forest");
  for (auto& p : f->parts) {
    const int rc = ti_forest_set_option(p.get(), option, value);
    if (rc) return rc;
  }
  std::lock_guard<std::mutex> lk(f->shap_mu);
  switch (option) {
    case TI_OPT_SHAP_TABLE_ROWS:
      if (value < 0) return fail(TI_ERR_INVALID, "TI_OPT_SHAP_TABLE_ROWS must be >= 0");
      f->shap_tab_rows = value;
      return TI_OK;
    case TI_OPT_SHAP_TABLE_MB:
      if (value < 0) return fail(TI_ERR_INVALID, "TI_OPT_SHAP_TABLE_MB must be >= 0");
      f->shap_tab_mb = value;
      return TI_OK;
    case TI_OPT_HOST_REGISTER:
      if (value != 0 && value != 1) return fail(TI_ERR_INVALID, "TI_OPT_HOST_REGISTER must be 0 or 1");
      f->host_register.store(static_cast<int32_t>(value));
      return TI_OK;
    case TI_OPT_LINEAR_SCRATCH_MB:
      if (value < 0) return fail(TI_ERR_INVALID, "TI_OPT_LINEAR_SCRATCH_MB must be >= 0");
      f->lin_scratch_mb.store(std::min<int64_t>(value, int64_t(1) << 30));
      return TI_OK;
    default:
      return fail(TI_ERR_INVALID, "unknown option " + std::to_string(option));
  }
}

int ti_output_shape(const ti_forest* f, int32_t kind, int64_t n_rows, int64_t* out_len,
                    int32_t* out_dtype) {
  if (!f || !out_len || !out_dtype) return fail(TI_ERR_INVALID, "null argument");
  if (kind < TI_OUTPUT_MARGIN || kind > TI_OUTPUT_CONTRIB_APPROX) return fail(TI_ERR_INVALID, "bad output kind");
  if (n_rows < 0) return fail(TI_ERR_INVALID, "negative n_rows");
  *out_len = n_rows * output_width(f, kind);
  *out_dtype = output_dtype(f, kind);
  return TI_OK;
}

static int check_call(const ti_forest* f, const void* X, int32_t xdt, int64_t rows, int32_t cols,
                      int64_t stride, int32_t kind, const void* out, int64_t out_len) {
  if (!f) return fail(TI_ERR_INVALID, "null forest");
  if (xdt != TI_F32 && xdt != TI_F64) return fail(TI_ERR_INVALID, "x_dtype must be TI_F32 or TI_F64");
  if (kind < TI_OUTPUT_MARGIN || kind > TI_OUTPUT_CONTRIB_APPROX) return fail(TI_ERR_INVALID, "bad output kind");
  if (rows < 0) return fail(TI_ERR_INVALID, "negative n_rows");
  if (rows == 0) return TI_OK;
  if (!X || !out) return fail(TI_ERR_INVALID, "null data pointer");
  if (cols <= 0) return fail(TI_ERR_INVALID, "n_cols must be > 0");
  if (stride < cols) return fail(TI_ERR_INVALID, "row_stride < n_cols");
  if (f->pre_steps > 0 && cols != f->F)
    return fail(TI_ERR_INVALID, "a forest with pre-steps needs n_cols == n_features (" +
                                    std::to_string(f->F) + "), got " + std::to_string(cols));
  if (out_len < rows * output_width(f, kind))
    return fail(TI_ERR_INVALID, "output buffer too small: need " +
                                    std::to_string(rows * output_width(f, kind)) + " elements");
  return TI_OK;
}

int ti_predict(ti_forest* f, const void* X, int32_t xdt, int64_t rows, int32_t cols,
               int64_t stride, int32_t kind, void* out, int64_t out_len) {
  int rc = check_call(f, X, xdt, rows, cols, stride, kind, out, out_len);
  if (rc || rows == 0) return rc;
  ti_forest* bf = base_forest(f);   // a chunked forest's parts share its device list
  const int nd = static_cast<int>(bf->devs.size());
  const size_t xs = dtype_size(xdt);
  const size_t os = dtype_size(output_dtype(f, kind)) * output_width(f, kind);
  const int64_t per = (rows + nd - 1) / nd;
  const unsigned char* xb = static_cast<const unsigned char*>(X);
  unsigned char* ob = static_cast<unsigned char*>(out);
  const bool hreg = bf->host_register.load() != 0;
  if (nd == 1)
    return predict_shard(f, 0, *bf->devs[0], xb, xdt, rows, cols, stride, kind, ob, hreg ? 1 : 0);
  // registered buffers (TI_OPT_HOST_REGISTER) with several devices: the whole
  // X and output are page-locked once here, before the shard threads start,
  // and unlocked after they join (shard threads registering their
  // own page-rounded slices shared boundary pages, and one thread's unregister
  // could unlock pages under another's in-flight DMA).  If either span cannot
  // be registered every shard takes the pinned staging chunks.
  HostSpan all_x, all_o;
  int reg_mode = 0;
  if (hreg && per > chunk_rows_for(f, xdt, stride, kind)) {
    const size_t x_bytes = static_cast<size_t>((rows - 1) * stride + cols) * xs;
    if (all_x.reg(xb, x_bytes, true) && all_o.reg(ob, static_cast<size_t>(rows) * os, true))
      reg_mode = 2;
  }
  std::vector<int> rcs(nd, TI_OK);
  std::vector<std::string> errs(nd);
  std::vector<std::thread> th;
  for (int i = 0; i < nd; ++i) {
    const int64_t r0 = per * i;
    const int64_t r1 = std::min(rows, r0 + per);
    if (r0 >= r1) break;
    th.emplace_back([&, i, r0, r1]() {
      rcs[i] = predict_shard(f, i, *bf->devs[i], xb + r0 * stride * xs, xdt, r1 - r0, cols, stride,
                             kind, ob + r0 * os, reg_mode);
      if (rcs[i]) errs[i] = g_last_error;
    });
  }
  for (auto& t : th) t.join();   // before all_x / all_o unregister
  for (int i = 0; i < nd; ++i)
    if (rcs[i]) return fail(rcs[i], "device slot " + std::to_string(i) + ": " + errs[i]);
  return TI_OK;
}

int ti_transform_device(ti_forest* f, int32_t slot, const void* margin, int64_t rows, void* out,
                        int64_t out_len, void* stream) {
  if (!f) return fail(TI_ERR_INVALID, "null forest");
  if (rows < 0) return fail(TI_ERR_INVALID, "negative row count");
  if (rows == 0) return TI_OK;
  if (!margin || !out) return fail(TI_ERR_INVALID, "null margin or output");
  if (margin == out) return fail(TI_ERR_INVALID, "margin and output must not alias");
  if (out_len < rows * output_width(f, TI_OUTPUT_PREDICT))
    return fail(TI_ERR_INVALID, "output buffer too small");
  ti_forest* bf = base_forest(f);
  if (slot < 0 || slot >= static_cast<int>(bf->devs.size()))
    return fail(TI_ERR_INVALID, "device_slot out of range");
  TI_HIP(hipSetDevice(bf->devs[slot]->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int threads = 256;
  const unsigned grid = static_cast<unsigned>((rows + threads - 1) / threads);
  if (f->accum == TI_F64)
    hipLaunchKernelGGL(transform_rows_kernel<double>, dim3(grid), dim3(threads), 0, s,
                       static_cast<const double*>(margin), rows, f->K, f->transform, f->tparam,
                       static_cast<double*>(out));
  else
    hipLaunchKernelGGL(transform_rows_kernel<float>, dim3(grid), dim3(threads), 0, s,
                       static_cast<const float*>(margin), rows, f->K, f->transform, f->tparam,
                       static_cast<float*>(out));
  TI_HIP(hipGetLastError());
  return TI_OK;
}

int ti_pretransform_device(ti_forest* f, int32_t slot, const void* X, int32_t xdt, int64_t rows,
                           int32_t cols, int64_t stride, float* out, void* stream) {
  if (!f) return fail(TI_ERR_INVALID, "null forest");
  if (xdt != TI_F32 && xdt != TI_F64) return fail(TI_ERR_INVALID, "x_dtype must be TI_F32 or TI_F64");
  if (rows < 0) return fail(TI_ERR_INVALID, "negative n_rows");
  if (rows == 0) return TI_OK;
  if (!X || !out) return fail(TI_ERR_INVALID, "null data pointer");
  if (cols != f->F)
    return fail(TI_ERR_INVALID, "n_cols must be the forest's n_features (" + std::to_string(f->F) + ")");
  if (stride < cols) return fail(TI_ERR_INVALID, "row_stride < n_cols");
  ti_forest* bf = base_forest(f);
  if (slot < 0 || slot >= static_cast<int>(bf->devs.size()))
    return fail(TI_ERR_INVALID, "device_slot out of range");
  DeviceForest& d = *bf->devs[slot];
  TI_HIP(hipSetDevice(d.device));
  return launch_pre_steps(d, f->pre_steps, X, xdt, rows, cols, stride, out,
                          static_cast<hipStream_t>(stream));
}

int ti_predict_device(ti_forest* f, int32_t slot, const void* X, int32_t xdt, int64_t rows,
                      int32_t cols, int64_t stride, int32_t kind, void* out, int64_t out_len,
                      void* stream) {
  int rc = check_call(f, X, xdt, rows, cols, stride, kind, out, out_len);
  if (rc || rows == 0) return rc;
  ti_forest* bf = base_forest(f);
  if (slot < 0 || slot >= static_cast<int>(bf->devs.size()))
    return fail(TI_ERR_INVALID, "device_slot out of range");
  DeviceForest& d = *bf->devs[slot];
  TI_HIP(hipSetDevice(d.device));
  return launch_any(f, slot, X, xdt, rows, cols, stride, kind, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
