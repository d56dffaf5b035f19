// treeinfer_approx.h — approximate (Saabas) contributions, TI_OUTPUT_CONTRIB_APPROX
// (ABI 8; xgboost's approx_contribs): the host tables (build_approx,
// ensure_approx) and the second of launch_approx's two stream-ordered passes
// (treeinfer.hip).  Included by treeinfer.hip alone.
//
// The attribution of a row depends on the leaf it reaches in each tree and on
// nothing else: the tree credits mean[child] - mean[node] to the split feature
// of every node on the path and mean[root] to the bias.  Pass 1 is the
// forest's own walk with TI_OUTPUT_LEAF into a [rows, T] int32 scratch, so
// every layout and every split rule is served by the kernel that predicts it.
// Pass 2, here, reads no X: per tree it looks up the reached leaf's record and
// adds the leaf's {column, delta} terms -- the path's deltas merged per
// feature on the host, in float64 -- into the row's accumulators.
//
// Tables (per replica, uploaded on the first call: ensure_approx):
//   leaf_base [T + 1]    first record of each tree (the kernel reads an id outside
//                        its tree's records as an empty record)
//   leaves    [sum over trees of (largest leaf id + 1)]  {begin, count}; tree
//                        t's record of the leaf whose library id is i sits at
//                        leaf_base[t] + i (ids that name no leaf own an empty
//                        record), so the ids need be neither dense nor node
//                        indexes, only non-negative and distinct within a tree
//   terms     [M]        {delta, column} in the path-arithmetic type (float32
//                        forests 8 bytes, float64 forests 16), column =
//                        group * (F + 1) + feature.  A vector leaf's term is
//                        laid out as K such entries, one a group, so the
//                        kernel has one term loop.
//   bias      [K]        base_margin * divisor + sum of the root means (float64)
//
// One lane per row, 64 rows a workgroup.  The accumulators are float64 for
// every forest (float32 forests round once, at the end, as TreeSHAP's generic
// kernel does), in LDS as [column][kApproxPitch] with the lane lowest: a wave's
// adds fall in distinct banks, and the transposed read of the epilogue
// (consecutive lanes, consecutive columns; pitch 65 doubles) does too.  A row
// wider than kApproxCols columns is split into column tiles over blockIdx.y; a
// tile walks every tree and skips the terms outside it under one unsigned
// compare.  Leaf ids are read as in linear_leaf_kernel: [R][32] blocks,
// coalesced, transposed through LDS.  A small batch is too few workgroups for
// the device: its trees are cut into slices of whole id chunks over blockIdx.z,
// whose raw float64 sums approx_slices_kernel adds in slice order.
#pragma once

#include "treeinfer_forest.h"

namespace ti {

constexpr int kApproxRows = 64;                  // rows per workgroup (one wave)
constexpr int kApproxPitch = kApproxRows + 1;    // doubles per accumulator column
constexpr int kApproxCols = 256;                 // accumulator columns a tile holds at most:
                                                 //   133,120 B + 8,448 B of leaf ids < 160 KiB

struct ApproxLeaf {   // one 8-byte load
  uint32_t begin;     // first term
  uint32_t count;     // terms
};
static_assert(sizeof(ApproxLeaf) == 8, "a leaf record is one global_load_dwordx2");

template <typename MT>
struct ApproxTerm;
template <>
struct ApproxTerm<float> {   // one 8-byte load
  float delta;
  uint32_t column;
};
template <>
struct alignas(16) ApproxTerm<double> {   // one 16-byte load
  double delta;
  uint32_t column;
  uint32_t pad;
};
static_assert(sizeof(ApproxTerm<float>) == 8 && sizeof(ApproxTerm<double>) == 16, "term sizes");

struct ApproxArgs {
  const int32_t* leaf_ids;     // [n_rows][T] pass 1's output for the rows of this launch
  const ApproxLeaf* leaves;
  const void* terms;           // ApproxTerm<MT>
  const int64_t* leaf_base;    // [T + 1]
  const double* bias;          // [K] before the divisor
  int64_t n_rows;
  int32_t n_trees;
  int32_t width;               // K * (F + 1)
  int32_t f1;                  // F + 1
  int32_t col_tile;            // columns per tile (<= kApproxCols)
  int32_t n_col_tiles;
  double divisor;
  void* out;                   // [n_rows][out_ld] OT
  int64_t out_ld;              // elements between output rows
  // tree slices (small batches): workgroup (x, y, z) walks id chunks
  // [z * slice_chunks, (z + 1) * slice_chunks) and, when part is set, writes its
  // raw float64 sums to part[z][row][column] for approx_slices_kernel
  int32_t slice_chunks;        // kLinTC-tree chunks a slice
  double* part;                // [slices][n_rows][width], or null: one slice, finished here
};

__device__ __forceinline__ void approx_load_term(const ApproxTerm<float>* p, double* delta, uint32_t* col) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  *delta = (double)__uint_as_float(w.x);
  *col = w.y;
}
__device__ __forceinline__ void approx_load_term(const ApproxTerm<double>* p, double* delta, uint32_t* col) {
  const u32x4 w = *reinterpret_cast<const u32x4*>(p);
  *delta = __hiloint2double((int)w.y, (int)w.x);
  *col = w.z;
}

template <typename MT, typename OT>
__global__ void __launch_bounds__(kApproxRows) approx_contrib_kernel(const ApproxArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int R = kApproxRows;
  constexpr int P = kApproxPitch;
  constexpr int kIlp = 4;   // leaf records in flight per lane
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const bool live = row0 + tid < a.n_rows;
  const int64_t left_rows = a.n_rows - row0;
  const int rows_here = left_rows < R ? (int)left_rows : R;
  const int T = a.n_trees;
  double* acc = reinterpret_cast<double*>(smem);   // [col_tile][P]
  int32_t* tile = reinterpret_cast<int32_t*>(smem + (size_t)a.col_tile * P * sizeof(double));   // [R][kLinPitch]
  const ApproxTerm<MT>* terms = static_cast<const ApproxTerm<MT>*>(a.terms);
  OT* out = static_cast<OT*>(a.out);

  for (int ct = blockIdx.y; ct < a.n_col_tiles; ct += gridDim.y) {
    const int c0 = ct * a.col_tile;
    const int wt = a.width - c0 < a.col_tile ? a.width - c0 : a.col_tile;
    __syncthreads();   // the previous tile's epilogue has read acc and the id chunk
    for (int e = tid; e < wt * P; e += R) acc[e] = 0.0;

    const int t_begin = (int)blockIdx.z * a.slice_chunks * kLinTC;
    const int t_end = T - t_begin < a.slice_chunks * kLinTC ? T : t_begin + a.slice_chunks * kLinTC;
    for (int t0 = t_begin; t0 < t_end; t0 += kLinTC) {
      const int tc = t_end - t0 < kLinTC ? t_end - t0 : kLinTC;
      if (t0 > t_begin) __syncthreads();   // the previous chunk has been read
      // coalesced [rows_here][tc] block -> transposed tile
      const int32_t* src = a.leaf_ids + row0 * (int64_t)T + t0;
      for (int e = tid; e < rows_here * kLinTC; e += R) {
        const int r = e / kLinTC;
        const int j = e - r * kLinTC;
        if (j < tc) tile[r * kLinPitch + j] = src[(int64_t)r * T + j];
      }
      __syncthreads();   // (the first chunk: acc is zeroed too)
      if (live) {
        for (int j0 = 0; j0 < tc; j0 += kIlp) {
          uint2 rec[kIlp];
#pragma unroll
          for (int u = 0; u < kIlp; ++u) {
            rec[u] = make_uint2(0u, 0u);
            if (j0 + u < tc) {
              const int64_t leaf = tile[tid * kLinPitch + j0 + u];
              const int64_t lb = a.leaf_base[t0 + j0 + u];
              if ((uint64_t)leaf < (uint64_t)(a.leaf_base[t0 + j0 + u + 1] - lb))
                rec[u] = *reinterpret_cast<const uint2*>(a.leaves + lb + leaf);
            }
          }
#pragma unroll
          for (int u = 0; u < kIlp; ++u) {   // trees in order: each column's sum has one order
            const ApproxTerm<MT>* tp = terms + rec[u].x;
            for (uint32_t i = 0; i < rec[u].y; ++i) {
              double delta;
              uint32_t col;
              approx_load_term(tp + i, &delta, &col);
              const uint32_t c = col - (uint32_t)c0;
              if (c < (uint32_t)wt) acc[c * P + tid] += delta;
            }
          }
        }
      }
    }
    __syncthreads();
    // the tile transposed: consecutive lanes write consecutive columns of a row
    for (int e = tid; e < rows_here * wt; e += R) {
      const int r = e / wt;
      const int c = e - r * wt;
      const int col = c0 + c;
      double v = acc[c * P + r];
      if (a.part != nullptr) {   // a slice's raw sums
        a.part[((int64_t)blockIdx.z * a.n_rows + row0 + r) * a.width + col] = v;
        continue;
      }
      const int g = col / a.f1;
      if (col - g * a.f1 == a.f1 - 1) v += a.bias[g];   // uniform over the rows: added once, here
      out[(row0 + r) * a.out_ld + col] = (OT)(v / a.divisor);
    }
  }
}

// The slices' partials summed in slice order, then the epilogue above: one
// thread an output element, consecutive threads consecutive columns of a row.
template <typename OT>
__global__ void __launch_bounds__(256) approx_slices_kernel(const ApproxArgs a, int slices) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_rows * a.width) return;
  const int64_t row = e / a.width;
  const int col = (int)(e - row * a.width);
  double v = 0.0;
  for (int z = 0; z < slices; ++z) v += a.part[(int64_t)z * a.n_rows * a.width + e];
  const int g = col / a.f1;
  if (col - g * a.f1 == a.f1 - 1) v += a.bias[g];
  static_cast<OT*>(a.out)[row * a.out_ld + col] = (OT)(v / a.divisor);
}

}  // namespace ti

namespace {

void free_approx(DeviceForest& d) {
  d.approx_mem.release();
  static_cast<ApproxPtrs&>(d) = ApproxPtrs();
}

// At create: whether approximate contributions are possible (covers, no linear
// leaves) and the host copy of the arrays build_approx reads on first use.
// keep_shap_source keeps one only where TreeSHAP is possible, and drops it once
// its own tables are resident; this one serves XGBoost-rule categorical forests
// too and needs the leaf ids.
void keep_approx_source(const ti_forest_desc* d, ti_forest* f) {
  f->approx_refused = d->lin_offset ? 2 : !d->cover ? 1 : 0;
  if (f->approx_refused) return;
  auto src = std::make_unique<ti_forest::ApproxSource>();
  const int64_t N = d->n_nodes, T = d->n_trees;
  src->tree_offset.assign(d->tree_offset, d->tree_offset + T + 1);
  if (d->tree_group) src->tree_group.assign(d->tree_group, d->tree_group + T);
  src->feature.assign(d->feature, d->feature + N);
  src->left.assign(d->left, d->left + N);
  src->right.assign(d->right, d->right + N);
  src->leaf_id.assign(d->leaf_id, d->leaf_id + N);
  src->leaf_value.assign(d->leaf_value, d->leaf_value + N * d->leaf_width);
  src->cover.assign(d->cover, d->cover + N);
  src->base_margin.assign(d->base_margin, d->base_margin + d->n_groups);
  f->approx_src = std::move(src);
}

struct ApproxTables {
  std::vector<int64_t> leaf_base;
  std::vector<ti::ApproxLeaf> leaves;
  std::vector<unsigned char> terms;   // ApproxTerm<MT>
  std::vector<double> bias;
};

template <typename MT>
void approx_push_term(std::vector<unsigned char>* terms, uint32_t column, double delta) {
  ti::ApproxTerm<MT> t{};
  t.delta = static_cast<MT>(delta);
  t.column = column;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(&t);
  terms->insert(terms->end(), p, p + sizeof(t));
}

// The tables of one forest.  Node means are xgboost's FillNodeMeanValues, the
// expression of ShapBuilder::mean (a node of zero cover divides by it, as the
// TreeSHAP bias does: its mean, and every delta and bias formed from it, is
// NaN or infinite); a path's deltas are merged per feature in path order, in
// float64, and then stored as MT.  No recursion: paths may be thousands deep.
template <typename MT>
int build_approx(const ti_forest* f, const ti_forest::ApproxSource& s, ApproxTables* out) {
  const int T = f->T, K = f->K, LW = f->LW, F1 = f->F + 1;
  out->leaf_base.assign(T + 1, 0);
  out->bias.assign(K, 0.0);
  for (int k = 0; k < K; ++k) out->bias[k] = s.base_margin[k] * f->divisor;
  std::vector<int32_t> order, parent, ids, chain, path_feat;
  std::vector<double> mean, path_delta;
  uint64_t n_terms = 0;
  for (int t = 0; t < T; ++t) {
    const int64_t b = s.tree_offset[t];
    const int32_t n = static_cast<int32_t>(s.tree_offset[t + 1] - b);
    // preorder from the root; parents come before their children
    order.clear();
    parent.assign(n, -1);
    order.push_back(0);
    for (size_t i = 0; i < order.size(); ++i) {
      const int32_t v = order[i];
      if (s.feature[b + v] < 0) continue;
      for (const int32_t c : {s.left[b + v], s.right[b + v]}) {
        parent[c] = v;
        order.push_back(c);
      }
    }
    mean.assign(static_cast<size_t>(n) * LW, 0.0);
    for (size_t i = order.size(); i-- > 0;) {
      const int32_t v = order[i];
      const int64_t g = b + v;
      double* m = &mean[static_cast<size_t>(v) * LW];
      if (s.feature[g] < 0) {
        for (int k = 0; k < LW; ++k) m[k] = s.leaf_value[g * LW + k];
        continue;
      }
      const int32_t l = s.left[g], r = s.right[g];
      for (int k = 0; k < LW; ++k)
        m[k] = (mean[static_cast<size_t>(l) * LW + k] * s.cover[b + l] +
                mean[static_cast<size_t>(r) * LW + k] * s.cover[b + r]) / s.cover[g];
    }
    if (LW == 1) out->bias[s.tree_group[t]] += mean[0];
    else for (int k = 0; k < K; ++k) out->bias[k] += mean[k];
    // the leaf ids TI_OUTPUT_LEAF reports: non-negative, distinct within the tree
    ids.clear();
    for (const int32_t v : order)
      if (s.feature[b + v] < 0) ids.push_back(s.leaf_id[b + v]);
    std::sort(ids.begin(), ids.end());
    if (ids.front() < 0 || std::adjacent_find(ids.begin(), ids.end()) != ids.end())
      return fail(TI_ERR_UNSUPPORTED,
                  "TI_OUTPUT_CONTRIB_APPROX finds a leaf's terms by its leaf id: tree " +
                      std::to_string(t) + " has leaf ids that are negative or not distinct");
    const size_t base = out->leaves.size();
    if (base + static_cast<size_t>(ids.back()) + 1 > std::numeric_limits<uint32_t>::max())
      return fail(TI_ERR_UNSUPPORTED, "TI_OUTPUT_CONTRIB_APPROX: the leaf ids span more than 2^32 records");
    out->leaf_base[t] = static_cast<int64_t>(base);
    out->leaves.resize(base + static_cast<size_t>(ids.back()) + 1, ti::ApproxLeaf{0, 0});
    out->leaf_base[t + 1] = static_cast<int64_t>(out->leaves.size());
    for (const int32_t v : order) {
      if (s.feature[b + v] < 0) {
        // root -> leaf, one entry a distinct feature in order of first occurrence
        path_feat.clear();
        path_delta.clear();
        chain.clear();   // the nodes from the leaf up
        for (int32_t u = v; u >= 0; u = parent[u]) chain.push_back(u);
        for (size_t i = chain.size(); i-- > 1;) {
          const int32_t node = chain[i], child = chain[i - 1];
          const int32_t fe = s.feature[b + node];
          size_t e = 0;
          while (e < path_feat.size() && path_feat[e] != fe) ++e;
          if (e == path_feat.size()) {
            path_feat.push_back(fe);
            path_delta.resize(path_delta.size() + LW, 0.0);
          }
          for (int k = 0; k < LW; ++k)
            path_delta[e * LW + k] += mean[static_cast<size_t>(child) * LW + k] -
                                      mean[static_cast<size_t>(node) * LW + k];
        }
        n_terms += path_feat.size() * static_cast<uint64_t>(LW);
        if (n_terms > std::numeric_limits<uint32_t>::max())
          return fail(TI_ERR_UNSUPPORTED, "TI_OUTPUT_CONTRIB_APPROX: more than 2^32 terms");
        ti::ApproxLeaf& rec = out->leaves[base + static_cast<size_t>(s.leaf_id[b + v])];
        rec.begin = static_cast<uint32_t>(out->terms.size() / sizeof(ti::ApproxTerm<MT>));
        rec.count = static_cast<uint32_t>(path_feat.size() * LW);
        for (size_t e = 0; e < path_feat.size(); ++e)
          for (int k = 0; k < LW; ++k) {
            const int grp = LW == 1 ? s.tree_group[t] : k;
            approx_push_term<MT>(&out->terms, static_cast<uint32_t>(grp * F1 + path_feat[e]),
                                 path_delta[e * LW + k]);
          }
      }
    }
  }
  return TI_OK;
}

// First TI_OUTPUT_CONTRIB_APPROX call of a handle: build the tables on the host
// and upload them to every replica, under the forest's lock (ensure_shap's
// lifecycle: predict-only serving pays nothing on the device, the bytes count
// in device_bytes, a failed upload frees every replica's tables and restores
// the counts; the host source stays for the retry and goes once they are
// resident).
int ensure_approx(ti_forest* f) {
  if (f->approx_ready.load(std::memory_order_acquire)) return TI_OK;
  std::lock_guard<std::mutex> lk(f->shap_mu);
  if (f->approx_ready.load(std::memory_order_relaxed)) return TI_OK;
  ApproxTables tab;
  int rc = f->accum == TI_F64 ? build_approx<double>(f, *f->approx_src, &tab)
                              : build_approx<float>(f, *f->approx_src, &tab);
  if (rc) return rc;
  int dev0 = 0;
  TI_HIP(hipGetDevice(&dev0));
  std::vector<int64_t> bytes0;
  for (auto& dp : f->devs) bytes0.push_back(dp->bytes);
  for (auto& dp : f->devs) {
    DeviceForest& d = *dp;
    if ((rc = fail_hip(hipSetDevice(d.device), "hipSetDevice"))) break;
    if ((rc = upload(&d.approx_mem, &d.approx_leaf_base, tab.leaf_base, &d.bytes)) ||
        (rc = upload(&d.approx_mem, &d.approx_leaves, tab.leaves, &d.bytes)) ||
        (rc = upload(&d.approx_mem, &d.approx_terms, tab.terms, &d.bytes)) ||
        (rc = upload(&d.approx_mem, &d.approx_bias, tab.bias, &d.bytes)))
      break;
  }
  if (rc) {
    const std::string err = g_last_error;
    for (size_t i = 0; i < f->devs.size(); ++i) {
      (void)hipSetDevice(f->devs[i]->device);
      free_approx(*f->devs[i]);
      f->devs[i]->bytes = bytes0[i];
    }
    (void)hipGetLastError();
    (void)hipSetDevice(dev0);
    return fail(rc, err);
  }
  TI_HIP(hipSetDevice(dev0));
  f->approx_src.reset();
  f->approx_ready.store(true, std::memory_order_release);
  return TI_OK;
}

}  // namespace
