// treeinfer_pack.h -- from a forest descriptor to a packed forest: validate,
// the model fields, one packer per layout, the planners of the record family
// and choose_layout, which tries them in order and commits one.  Host
// arithmetic only: nothing here makes a HIP runtime call.  Included by
// treeinfer.hip alone.
#pragma once

#include "treeinfer_forest.h"

namespace {

// -------------------------------------------------------------- validation
int validate(const ti_forest_desc* d, std::vector<int>* depth_out) {
  if (!d) return fail(TI_ERR_INVALID, "null forest descriptor");
  if (d->abi_version != TI_ABI_VERSION)
    return fail(TI_ERR_INVALID, "abi_version mismatch: got " + std::to_string(d->abi_version));
  if (d->n_trees <= 0) return fail(TI_ERR_INVALID, "n_trees must be > 0");
  if (d->n_features <= 0 || d->n_features > (1 << 24))
    return fail(TI_ERR_INVALID, "n_features out of range");
  if (d->n_groups <= 0) return fail(TI_ERR_INVALID, "n_groups must be > 0");
  if (d->n_groups > (1 << 20)) return fail(TI_ERR_UNSUPPORTED, "n_groups > 2^20");
  if (d->leaf_width != 1 && d->leaf_width != d->n_groups)
    return fail(TI_ERR_INVALID, "leaf_width must be 1 or n_groups");
  if (d->accum_dtype != TI_F32 && d->accum_dtype != TI_F64)
    return fail(TI_ERR_INVALID, "accum_dtype must be TI_F32 or TI_F64");
  if (d->transform < TI_TRANSFORM_IDENTITY || d->transform > TI_TRANSFORM_STEP)
    return fail(TI_ERR_INVALID, "unknown transform");
  if (!(d->average_divisor > 0.0)) return fail(TI_ERR_INVALID, "average_divisor must be > 0");
  if (!d->tree_offset || !d->feature || !d->threshold || !d->flags || !d->left || !d->right ||
      !d->leaf_id || !d->leaf_value || !d->base_margin)
    return fail(TI_ERR_INVALID, "null array in forest descriptor");
  if (d->leaf_width == 1 && !d->tree_group) return fail(TI_ERR_INVALID, "null tree_group");
  if (d->tree_offset[0] != 0 || d->tree_offset[d->n_trees] != d->n_nodes)
    return fail(TI_ERR_INVALID, "tree_offset must start at 0 and end at n_nodes");
  if (d->lin_offset) {   // linear leaves (ABI 6)
    if (d->leaf_width != 1)
      return fail(TI_ERR_INVALID, "linear leaves need leaf_width == 1");
    if (d->accum_dtype != TI_F64)
      return fail(TI_ERR_INVALID, "linear leaves need float64 sums (accum_dtype TI_F64)");
    if (!d->lin_const) return fail(TI_ERR_INVALID, "linear leaves without lin_const");
    if (d->n_lin_terms < 0 || d->n_lin_terms > 0xffffffffLL)
      return fail(TI_ERR_INVALID, "n_lin_terms out of range");
    if (d->n_lin_terms > 0 && (!d->lin_feature || !d->lin_coeff))
      return fail(TI_ERR_INVALID, "linear terms without lin_feature / lin_coeff");
    if (d->lin_offset[0] != 0 || d->lin_offset[d->n_nodes] != d->n_lin_terms)
      return fail(TI_ERR_INVALID, "lin_offset must start at 0 and end at n_lin_terms");
    for (int64_t n = 0; n < d->n_nodes; ++n)
      if (d->lin_offset[n + 1] < d->lin_offset[n])
        return fail(TI_ERR_INVALID, "lin_offset must not decrease");
    for (int64_t i = 0; i < d->n_lin_terms; ++i)
      if (d->lin_feature[i] < 0 || d->lin_feature[i] >= d->n_features)
        return fail(TI_ERR_INVALID, "lin_feature out of [0, n_features)");
    if (d->n_groups > ti::kMaxGroups)
      return fail(TI_ERR_UNSUPPORTED,
                  "linear leaves with more than 16 output groups: such forests are split into "
                  "group parts, and the linear tables are not subset per part");
  }
  if (d->n_pre_steps < 0) return fail(TI_ERR_INVALID, "n_pre_steps must be >= 0");
  if (d->n_pre_steps > 0) {   // pre-steps (ABI 9)
    if (!d->pre_op || !d->pre_const) return fail(TI_ERR_INVALID, "pre-steps without pre_op / pre_const");
    if (d->n_pre_steps > TI_PRE_MAX_STEPS)
      return fail(TI_ERR_UNSUPPORTED, "more than " + std::to_string(TI_PRE_MAX_STEPS) + " pre-steps");
    for (int s = 0; s < d->n_pre_steps; ++s)
      if (d->pre_op[s] < TI_PRE_FILL_NAN || d->pre_op[s] > TI_PRE_ADD)
        return fail(TI_ERR_INVALID, "unknown pre-step op code " + std::to_string(d->pre_op[s]));
    if (d->lin_offset)
      return fail(TI_ERR_UNSUPPORTED,
                  "pre-steps with linear leaves (the linear models would read the raw columns; no "
                  "loader produces the combination)");
  }
  depth_out->assign(d->n_trees, 0);
  std::vector<int> stack_node, stack_depth;
  for (int t = 0; t < d->n_trees; ++t) {
    const int64_t b = d->tree_offset[t], e = d->tree_offset[t + 1];
    if (e <= b) return fail(TI_ERR_INVALID, "tree " + std::to_string(t) + " has no nodes");
    if (e - b > (int64_t(1) << 30)) return fail(TI_ERR_INVALID, "tree too large");
    const int32_t n = static_cast<int32_t>(e - b);
    if (d->leaf_width == 1 && (d->tree_group[t] < 0 || d->tree_group[t] >= d->n_groups))
      return fail(TI_ERR_INVALID, "tree_group out of range in tree " + std::to_string(t));
    int max_depth = 0;
    int64_t visited = 0;
    stack_node.assign(1, 0);
    stack_depth.assign(1, 0);
    while (!stack_node.empty()) {
      const int v = stack_node.back(), dep = stack_depth.back();
      stack_node.pop_back();
      stack_depth.pop_back();
      if (++visited > n) return fail(TI_ERR_INVALID, "cycle in tree " + std::to_string(t));
      const int64_t g = b + v;
      if (d->feature[g] < 0) {
        max_depth = std::max(max_depth, dep);
        continue;
      }
      if (d->feature[g] >= d->n_features)
        return fail(TI_ERR_INVALID, "split feature >= n_features in tree " + std::to_string(t));
      if ((d->flags[g] & TI_NODE_CAT_XGB) && !(d->flags[g] & TI_NODE_CATEGORICAL))
        return fail(TI_ERR_INVALID, "TI_NODE_CAT_XGB without TI_NODE_CATEGORICAL in tree " +
                                        std::to_string(t));
      if (d->flags[g] & TI_NODE_CATEGORICAL) {
        if (!d->cat_bits || !d->cat_offset || !d->cat_nwords)
          return fail(TI_ERR_INVALID, "categorical node without cat_bits/cat_offset/cat_nwords");
        const int64_t o = d->cat_offset[g], w = d->cat_nwords[g];
        if (o < 0 || w < 0 || o + w > d->n_cat_words)
          return fail(TI_ERR_INVALID, "categorical bitset out of range in tree " + std::to_string(t));
      }
      const int32_t l = d->left[g], r = d->right[g];
      if (l < 0 || l >= n || r < 0 || r >= n)
        return fail(TI_ERR_INVALID, "child index out of range in tree " + std::to_string(t));
      if (dep + 1 > 64) return fail(TI_ERR_UNSUPPORTED, "tree deeper than 64");
      stack_node.push_back(l);
      stack_depth.push_back(dep + 1);
      stack_node.push_back(r);
      stack_depth.push_back(dep + 1);
    }
    (*depth_out)[t] = max_depth;
  }
  return TI_OK;
}

// ------------------------------------------------------------ model fields
// The forest's model scalars, from a validated descriptor and its tree depths.
// ti_forest_create and create_chunked both start here (a chunked parent keeps
// its bases in the parts: base[] holds kMaxGroups).
void fill_model(const ti_forest_desc* desc, const std::vector<int>& depth, ti_forest* f) {
  f->T = desc->n_trees;
  f->F = desc->n_features;
  f->K = desc->n_groups;
  f->LW = desc->leaf_width;
  f->accum = desc->accum_dtype;
  f->base_first = desc->base_first ? 1 : 0;
  f->lgb_zero_map = desc->lgb_zero_map ? 1 : 0;
  f->transform = desc->transform;
  f->tparam = desc->transform_param;
  f->divisor = desc->average_divisor;
  if (f->K <= ti::kMaxGroups)
    for (int k = 0; k < f->K; ++k) f->base[k] = desc->base_margin[k];
  for (int64_t i = 0; i < desc->n_nodes; ++i)
    if (desc->feature[i] >= 0) {
      if (desc->flags[i] & TI_NODE_CATEGORICAL) {
        f->has_cat = 1;
        if (desc->flags[i] & TI_NODE_CAT_XGB) f->has_cat_xgb = 1;
        else f->has_cat_lgb = 1;
      }
      else if (desc->flags[i] & TI_NODE_ZERO_FLIP) f->zero_rule = 1;
    }
  f->linear = desc->lin_offset ? 1 : 0;
  f->pre_steps = desc->n_pre_steps;
  f->depth = *std::max_element(depth.begin(), depth.end());
}

// The packers are templates over the input view XT and the accumulator ACC.
// with_acc calls fn(ACC{}) for the forest's accumulator; for_views calls
// fn(XT{}, ACC{}, view) for the float32 view (0), then the float64 view (1),
// and stops at the first false.
template <typename Fn>
auto with_acc(int accum, Fn fn) {
  return accum == TI_F64 ? fn(double{}) : fn(float{});
}
template <typename Fn>
bool for_views(int accum, Fn fn) {
  return with_acc(accum, [&](auto acc) { return fn(float{}, acc, 0) && fn(double{}, acc, 1); });
}

// ------------------------------------------------------------ heap packing
template <typename XT, typename ACC>
void pack_heap(const ti_forest_desc* d, int D, int64_t stride, uint32_t feat_scale,
               std::vector<unsigned char>* img, std::vector<int32_t>* leaf_ids) {
  using Node = HeapNode<XT>;
  const int NI = (1 << D) - 1, NL = 1 << D, LW = d->leaf_width;
  img->assign(static_cast<size_t>(stride) * d->n_trees, 0);
  if (leaf_ids) leaf_ids->assign(static_cast<size_t>(NL) * d->n_trees, 0);
  struct Item { int32_t node; int32_t heap; int32_t level; };
  std::vector<Item> st;
  for (int t = 0; t < d->n_trees; ++t) {
    unsigned char* rec = img->data() + static_cast<size_t>(stride) * t;
    Node* nodes = reinterpret_cast<Node*>(rec);
    ACC* leaves = reinterpret_cast<ACC*>(rec + sizeof(Node) * NI);
    const int64_t b = d->tree_offset[t];
    st.assign(1, Item{0, 0, 0});
    while (!st.empty()) {
      const Item it = st.back();
      st.pop_back();
      const int64_t g = b + it.node;
      if (it.level == D) {   // leaf slot
        const int slot = it.heap - NI;
        for (int k = 0; k < LW; ++k)
          leaves[static_cast<size_t>(slot) * LW + k] = static_cast<ACC>(d->leaf_value[g * LW + k]);
        if (leaf_ids) (*leaf_ids)[static_cast<size_t>(t) * NL + slot] = d->leaf_id[g];
        continue;
      }
      Node nd{};
      if (d->feature[g] < 0) {   // shallow leaf: pad with always-left nodes
        nd.thr = static_cast<decltype(nd.thr)>(INFINITY);
        nd.meta = kPadMeta;
        nodes[it.heap] = nd;
        st.push_back(Item{it.node, 2 * it.heap + 1, it.level + 1});
        st.push_back(Item{it.node, 2 * it.heap + 2, it.level + 1});
      } else {
        if (sizeof(XT) == 4)
          nd.thr = static_cast<decltype(nd.thr)>(round_down_f32(d->threshold[g]));
        else
          nd.thr = static_cast<decltype(nd.thr)>(d->threshold[g]);
        nd.meta = make_meta(static_cast<int32_t>(d->feature[g] * feat_scale), d->flags[g]);
        nodes[it.heap] = nd;
        st.push_back(Item{d->left[g], 2 * it.heap + 1, it.level + 1});
        st.push_back(Item{d->right[g], 2 * it.heap + 2, it.level + 1});
      }
    }
  }
}

// ---------------------------------------------------- categorical heap packing
// Layout 10 (treeinfer_cheap.h): pack_heap's record with the tree's bitsets
// behind the leaves.  A categorical node's thr field holds the u32-word offset,
// from the start of its tree's block, of its run [nwords, w0, w1, ...] in its
// low 16 bits and nwords again in the next 16 (plan_cheap: a block is at most
// kPf x 16 x R <= 64 KB).
template <typename XT>
int64_t cheap_block_bytes(const ti_forest_desc* d, int D, size_t acc_sz, int t) {
  const int NI = (1 << D) - 1, NL = 1 << D;
  int64_t words = 0;
  for (int64_t g = d->tree_offset[t]; g < d->tree_offset[t + 1]; ++g)
    if (d->feature[g] >= 0 && (d->flags[g] & TI_NODE_CATEGORICAL)) words += 1 + d->cat_nwords[g];
  return static_cast<int64_t>(sizeof(HeapNode<XT>)) * NI +
         static_cast<int64_t>(acc_sz) * NL * d->leaf_width + 4 * words;
}

template <typename XT>
int64_t cheap_stride(const ti_forest_desc* d, int D, size_t acc_sz) {
  int64_t m = 0;
  for (int t = 0; t < d->n_trees; ++t) m = std::max(m, cheap_block_bytes<XT>(d, D, acc_sz, t));
  return static_cast<int64_t>(align16(static_cast<size_t>(m)));
}

template <typename XT, typename ACC>
void pack_cheap(const ti_forest_desc* d, int D, int64_t stride, uint32_t feat_scale,
                std::vector<unsigned char>* img, std::vector<int32_t>* leaf_ids) {
  using Node = HeapNode<XT>;
  pack_heap<XT, ACC>(d, D, stride, feat_scale, img, leaf_ids);
  const int NI = (1 << D) - 1, NL = 1 << D, LW = d->leaf_width;
  const uint32_t words0 =
      static_cast<uint32_t>((sizeof(Node) * NI + sizeof(ACC) * NL * LW) / sizeof(uint32_t));
  struct Item { int32_t node; int32_t heap; };
  std::vector<Item> st;
  for (int t = 0; t < d->n_trees; ++t) {
    unsigned char* rec = img->data() + static_cast<size_t>(stride) * t;
    Node* nodes = reinterpret_cast<Node*>(rec);
    uint32_t* words = reinterpret_cast<uint32_t*>(rec);
    uint32_t at = words0;
    const int64_t b = d->tree_offset[t];
    st.assign(1, Item{0, 0});
    while (!st.empty()) {
      const Item it = st.back();
      st.pop_back();
      const int64_t g = b + it.node;
      if (d->feature[g] < 0) continue;   // a leaf: pack_heap padded below it
      if (d->flags[g] & TI_NODE_CATEGORICAL) {
        const int32_t nw = d->cat_nwords[g];
        Node nd{};
        // low word of the thr field (little endian): run offset | nwords << 16
        const uint32_t ref = at | (static_cast<uint32_t>(nw) << 16);
        std::memcpy(&nd.thr, &ref, sizeof(ref));
        nd.meta = make_cat_meta(static_cast<uint32_t>(d->feature[g]) * feat_scale, d->flags[g]);
        nodes[it.heap] = nd;
        words[at++] = static_cast<uint32_t>(nw);
        for (int32_t w = 0; w < nw; ++w) words[at++] = d->cat_bits[d->cat_offset[g] + w];
      }
      st.push_back(Item{d->left[g], 2 * it.heap + 1});
      st.push_back(Item{d->right[g], 2 * it.heap + 2});
    }
  }
}

// -------------------------------------------------------- explicit packing
// Hot nodes first: the nodes of one tree level (tree-local indices, tree's
// first node b) ordered by cover, largest first (stable: breadth-first order
// among equals), when the model carries covers (xgboost sum_hess, LightGBM
// counts, sklearn weighted_n_node_samples) and TI_COVER_ORDER is not 0.  The
// lanes of a wave take the paths the training rows took, so at each step of a
// lockstep walk they crowd onto the high-cover nodes of a level: packed
// together, those share 128-byte lines (a gather's cost is its distinct lines:
// C4 7.3 instead of 12.5 lines a gather over N(0,1) rows, simulated) and LDS
// dwords (broadcast, not bank conflicts).  Layout only: results are unchanged.
void cover_order(const ti_forest_desc* d, int64_t b, std::vector<int32_t>* level) {
  if (!d->cover || env_int("TI_COVER_ORDER", 1) == 0) return;
  const double* c = d->cover + b;
  std::stable_sort(level->begin(), level->end(),
                   [c](int32_t x, int32_t y) { return c[x] > c[y]; });
}

// The leaves of a tree in level order, each level's by cover (cover_order):
// the leaf numbering of pack_explicit and of the record layouts' leaf slots.
void leaf_order(const ti_forest_desc* d, int64_t b, std::vector<int32_t>* out) {
  out->clear();
  std::vector<int32_t> level(1, 0), next;
  while (!level.empty()) {
    cover_order(d, b, &level);
    next.clear();
    for (const int32_t v : level) {
      const int64_t g = b + v;
      if (d->feature[g] < 0) {
        out->push_back(v);
      } else {
        next.push_back(d->left[g]);
        next.push_back(d->right[g]);
      }
    }
    level.swap(next);
  }
}

template <typename ACC>
void pack_explicit(const ti_forest_desc* d, HostImage* h) {   // a fresh image
  const int LW = d->leaf_width;
  h->node_base.assign(d->n_trees, 0);
  h->leaf_base.assign(d->n_trees, 0);
  h->root.assign(d->n_trees, 0);
  std::vector<ACC> leaves;
  std::vector<int32_t> remap;
  std::vector<int32_t> queue, lorder;
  for (int t = 0; t < d->n_trees; ++t) {
    const int64_t b = d->tree_offset[t];
    const int32_t n = static_cast<int32_t>(d->tree_offset[t + 1] - b);
    remap.assign(n, 0);
    const int64_t nb = static_cast<int64_t>(h->nodes.size());
    const int64_t lb = static_cast<int64_t>(h->exp_leaf_ids.size());
    h->node_base[t] = nb;
    h->leaf_base[t] = lb;
    // leaves numbered level by level, the level's by cover (leaf_order: the
    // record layouts' leaf slots follow the same order, so one leaf table
    // serves every layout); internal nodes breadth-first: the top levels of a
    // tree share cache lines
    leaf_order(d, b, &lorder);
    for (size_t i = 0; i < lorder.size(); ++i) {
      const int64_t g = b + lorder[i];
      remap[lorder[i]] = ~static_cast<int32_t>(i);
      h->exp_leaf_ids.push_back(d->leaf_id[g]);
      for (int k = 0; k < LW; ++k) leaves.push_back(static_cast<ACC>(d->leaf_value[g * LW + k]));
    }
    queue.assign(1, 0);
    int32_t n_int = 0;
    for (size_t qi = 0; qi < queue.size(); ++qi) {
      const int32_t v = queue[qi];
      const int64_t g = b + v;
      if (d->feature[g] < 0) continue;
      remap[v] = n_int++;
      queue.push_back(d->left[g]);
      queue.push_back(d->right[g]);
    }
    h->nodes.resize(nb + n_int);
    h->thr64.resize(nb + n_int);
    h->exp_src.resize(nb + n_int);
    for (size_t qi = 0; qi < queue.size(); ++qi) {
      const int32_t v = queue[qi];
      const int64_t g = b + v;
      if (d->feature[g] < 0) continue;
      ExpNode e;
      e.thr = round_down_f32(d->threshold[g]);
      e.meta = make_meta(d->feature[g], d->flags[g]);
      if (d->flags[g] & TI_NODE_CATEGORICAL) {
        // threshold slot carries the word offset of [nwords, bitset...]
        const uint32_t at = static_cast<uint32_t>(h->cat_words.size());
        const int32_t nw = d->cat_nwords[g];
        h->cat_words.push_back(static_cast<uint32_t>(nw));
        for (int32_t w = 0; w < nw; ++w) h->cat_words.push_back(d->cat_bits[d->cat_offset[g] + w]);
        std::memcpy(&e.thr, &at, sizeof(at));
        e.meta = make_cat_meta(static_cast<uint32_t>(d->feature[g]), d->flags[g]);
      }
      e.left = remap[d->left[g]];
      e.right = remap[d->right[g]];
      h->nodes[nb + remap[v]] = e;
      h->thr64[nb + remap[v]] = d->threshold[g];
      h->exp_src[nb + remap[v]] = g;
    }
    h->root[t] = remap[0];
  }
  h->leaves.resize(leaves.size() * sizeof(ACC));
  if (!leaves.empty()) std::memcpy(h->leaves.data(), leaves.data(), h->leaves.size());
}


// ------------------------------------------------------ binned heap packing
// Rank binning (treeinfer_kernels.h, stage_bins): per feature the sorted
// distinct thresholds of the XT view, an Eytzinger search table of 2^L
// entries (1-based, +inf padded) and per-node ranks.  Returns false when the
// forest does not qualify (too many distinct thresholds, or a feature image
// whose offsets overflow the node's 15 bits even at 64-row tiles).
template <typename XT>
XT threshold_view(double t) {
  if (sizeof(XT) == 4) return static_cast<XT>(round_down_f32(t));
  return static_cast<XT>(t);
}

void eytzinger_fill(const std::vector<double>& sorted, std::vector<double>* out, size_t k, size_t* i) {
  if (k >= out->size()) return;
  eytzinger_fill(sorted, out, 2 * k, i);
  (*out)[k] = *i < sorted.size() ? sorted[*i] : INFINITY;
  ++*i;
  eytzinger_fill(sorted, out, 2 * k + 1, i);
}

// Per-feature rank tables of one XT view.  With zero_bins, every feature
// that a LightGBM zero-missing node tests also gets the thresholds {-denorm_min,
// 0}: then exactly x == 0 (+-0) falls in the bin 1 + index(0) (zbin), so the
// zero rule becomes an integer compare as well.
template <typename XT>
struct RankTables {
  std::vector<std::vector<XT>> u;   // sorted distinct thresholds per feature
  std::vector<uint32_t> zbin;       // bin of exact 0 per feature (0: none)
  size_t m_max = 0;
  int L = 0;

  uint32_t rank(int f, double thr) const {
    const XT t = threshold_view<XT>(thr);
    if (std::isnan(static_cast<double>(t))) return 0;   // NaN threshold: never left
    return 1u + static_cast<uint32_t>(std::lower_bound(u[f].begin(), u[f].end(), t) - u[f].begin());
  }
};

template <typename XT>
RankTables<XT> collect_ranks(const ti_forest_desc* d, bool zero_bins) {
  RankTables<XT> rt;
  const int F = d->n_features;
  rt.u.assign(F, {});
  rt.zbin.assign(F, 0);
  std::vector<char> zf(F, 0);
  for (int64_t g = 0; g < d->n_nodes; ++g) {
    if (d->feature[g] < 0 || (d->flags[g] & TI_NODE_CATEGORICAL)) continue;
    const XT t = threshold_view<XT>(d->threshold[g]);
    if (!std::isnan(static_cast<double>(t))) rt.u[d->feature[g]].push_back(t);
    if (zero_bins && (d->flags[g] & TI_NODE_ZERO_FLIP)) zf[d->feature[g]] = 1;
  }
  for (int f = 0; f < F; ++f) {
    auto& v = rt.u[f];
    if (zf[f]) {
      v.push_back(XT(0));
      v.push_back(-std::numeric_limits<XT>::denorm_min());
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    rt.m_max = std::max(rt.m_max, v.size());
    if (zf[f]) rt.zbin[f] = 1u + static_cast<uint32_t>(std::lower_bound(v.begin(), v.end(), XT(0)) - v.begin());
  }
  while ((static_cast<size_t>(1) << rt.L) - 1 < rt.m_max) ++rt.L;
  return rt;
}

// [F][2^L] Eytzinger search tables (1-based, +inf padded) as XT bytes.
template <typename XT>
void eytzinger_tables(const RankTables<XT>& rt, std::vector<unsigned char>* out) {
  const int F = static_cast<int>(rt.u.size());
  const size_t tsz = static_cast<size_t>(1) << rt.L;
  out->assign(static_cast<size_t>(F) * tsz * sizeof(XT), 0);
  XT* tbl = reinterpret_cast<XT*>(out->data());
  std::vector<double> srt, ey(tsz);
  for (int f = 0; f < F; ++f) {
    srt.assign(rt.u[f].begin(), rt.u[f].end());
    size_t i = 0;
    std::fill(ey.begin(), ey.end(), static_cast<double>(INFINITY));
    eytzinger_fill(srt, &ey, 1, &i);
    for (size_t k = 0; k < tsz; ++k) tbl[f * tsz + k] = static_cast<XT>(ey[k]);
  }
}

// 5-ary search tables (float32 view of layouts 6-9, rx_stage_bins): per
// feature a complete 5-ary tree of height H, node j (0-based, children
// 5j+1 .. 5j+5) holding 4 keys, filled in order with the sorted thresholds and
// +inf padding.  The search counts the keys below x at each node and descends;
// after H levels, j - (5^H - 1)/4 = #{u < x}: the same rank as the Eytzinger
// search, in H 16-byte gathers instead of L 4-byte ones.
template <typename XT>
void kary_fill(const std::vector<XT>& srt, std::vector<XT>* out, size_t j, int level, int H,
               size_t* i) {
  if (level == H) return;
  for (int c = 0; c < 4; ++c) {
    kary_fill(srt, out, 5 * j + 1 + c, level + 1, H, i);
    (*out)[4 * j + c] = *i < srt.size() ? srt[*i] : static_cast<XT>(INFINITY);
    ++*i;
  }
  kary_fill(srt, out, 5 * j + 5, level + 1, H, i);
}

// (float32 view: 16-byte nodes; float64 view: 32-byte nodes of 4 doubles)
template <typename XT>
void kary_tables(const RankTables<XT>& rt, std::vector<unsigned char>* out, int* height) {
  const int F = static_cast<int>(rt.u.size());
  int H = 1;
  size_t p5 = 5;
  while (p5 - 1 < rt.m_max) {
    p5 *= 5;
    ++H;
  }
  const size_t nn = (p5 - 1) / 4;
  out->assign(static_cast<size_t>(F) * nn * 4 * sizeof(XT), 0);
  std::vector<XT> node(nn * 4), srt;
  for (int f = 0; f < F; ++f) {
    srt.assign(rt.u[f].begin(), rt.u[f].end());
    size_t i = 0;
    kary_fill(srt, &node, 0, 0, H, &i);
    std::memcpy(out->data() + static_cast<size_t>(f) * nn * 4 * sizeof(XT), node.data(),
                nn * 4 * sizeof(XT));
  }
  *height = H;
}

// Bucket tables (float32 view of the binned heap, rank_search): per feature
// {lo, scale, first key, 0}, then start[F][NB] u16, then every feature's
// sorted thresholds followed by 4 +inf.  lo is the smallest threshold, scale =
// NB / (hi - lo) (0 for a feature with fewer than two thresholds: one bucket),
// and start[k] counts the thresholds whose ti::bin_bucket is below k -- the
// same float32 operations the device applies to x, so the thresholds of lower
// buckets are < x and those of higher buckets >= x for every x, and the 4 keys
// from start[bucket(x)] on decide the rank.  NB, one per forest, is the first
// power of two from the largest threshold count up to 4,096 at which no
// bucket holds more than 4 thresholds.  Returns false, leaving *out alone,
// when there is none, when 2 gathers are no fewer than the 5-ary tree's
// (H <= 2), or when a feature's hi - lo overflows or its scale is not a
// positive finite float.  One load of 4 keys is a measured bound: every bucket
// gather is divergent, while the 5-ary tree's top three levels sit in a few
// cache lines, so with 3 loads (C2: 4,794 thresholds in 4,096 buckets, 12 in
// the fullest) the texture addresser's time doubled and the kernel lost 9 %;
// with one (c2_hist) it gains 2 %.
// start[F][NB] at NB buckets and the fullest bucket's count; < 0 when some
// feature's span or scale is unusable.
int bucket_starts(const RankTables<float>& rt, int NB, std::vector<float>* ls,
                  std::vector<uint16_t>* start) {
  const int F = static_cast<int>(rt.u.size());
  ls->assign(static_cast<size_t>(F) * 2, 0.0f);
  start->assign(static_cast<size_t>(F) * NB, 0);
  std::vector<size_t> cnt;
  size_t occ_max = 0;
  for (int f = 0; f < F; ++f) {
    const std::vector<float>& u = rt.u[f];
    float lo = 0.0f, scale = 0.0f;
    if (!u.empty()) lo = u.front();
    if (u.size() > 1) {
      const float span = u.back() - lo;
      scale = static_cast<float>(NB) / span;
      if (!std::isfinite(span) || !std::isfinite(scale) || !(scale > 0.0f)) return -1;
    }
    (*ls)[2 * f] = lo;
    (*ls)[2 * f + 1] = scale;
    cnt.assign(NB, 0);
    for (float t : u) ++cnt[ti::bin_bucket(t, lo, scale, NB)];
    size_t below = 0;
    for (int k = 0; k < NB; ++k) {
      (*start)[static_cast<size_t>(f) * NB + k] = static_cast<uint16_t>(below);
      below += cnt[k];
      occ_max = std::max(occ_max, cnt[k]);
    }
  }
  return static_cast<int>(occ_max);
}

bool bucket_tables(const RankTables<float>& rt, std::vector<unsigned char>* out, int* nb_out) {
  const int F = static_cast<int>(rt.u.size());
  if (rt.m_max <= 24) return false;   // the 5-ary tree has H <= 2 levels: two gathers already
  int NB = 2;
  while (NB < 4096 && static_cast<size_t>(NB) < rt.m_max) NB *= 2;
  std::vector<float> ls;
  std::vector<uint16_t> start;
  int occ = bucket_starts(rt, NB, &ls, &start);
  while (occ > 4 && NB < 4096) occ = bucket_starts(rt, NB *= 2, &ls, &start);
  if (occ < 0 || occ > 4) return false;
  struct Feat { float lo, scale; uint32_t first, pad; };
  size_t keys = 0;
  for (int f = 0; f < F; ++f) keys += rt.u[f].size() + 4;
  const size_t b_fs = static_cast<size_t>(F) * sizeof(Feat), b_st = start.size() * sizeof(uint16_t);
  out->assign(b_fs + b_st + keys * sizeof(float), 0);
  Feat* fs = reinterpret_cast<Feat*>(out->data());
  std::memcpy(out->data() + b_fs, start.data(), b_st);
  float* srt = reinterpret_cast<float*>(out->data() + b_fs + b_st);
  size_t at = 0;
  for (int f = 0; f < F; ++f) {
    fs[f] = Feat{ls[2 * f], ls[2 * f + 1], static_cast<uint32_t>(at), 0u};
    at = std::copy(rt.u[f].begin(), rt.u[f].end(), srt + at) - srt;
    std::fill(srt + at, srt + at + 4, INFINITY);
    at += 4;
  }
  *nb_out = NB;
  return true;
}

// The fixed walk (bheap_fix_kernel) finds a node's children pair through the
// pair slot the node word carries in bits 3..10, not by heap arithmetic, so
// within a level the slots may be any permutation.  fix_permute numbers each
// level's nodes by cover, largest first: the lanes of a wave, which crowd onto
// the nodes the training rows took, then read pairs packed at the start of the
// level's slots -- the same address (a broadcast) or nearby dwords -- instead
// of pairs up to 1 KB apart whose dwords collide in the LDS banks.  Same
// words, same walk, same sums; only the fixed walk reads this image (leaf ids
// keep the heap-indexed walk on img).  `spread` (the default; TI_FIX_SPREAD=0
// numbers every level sequentially) balances the levels of more than 32 pairs
// over the bank classes, below.
void fix_permute(BinImage* bi, const std::vector<double>& hcov, int NE, bool spread) {
  constexpr int kCls = 32;   // pair slots per sweep of the 64 LDS banks
  const int64_t T = static_cast<int64_t>(bi->img.size()) / bi->stride;
  bi->fix_img.assign(bi->img.size(), 0);
  std::vector<int32_t> pi(NE, 0), lvl;
  for (int64_t t = 0; t < T; ++t) {
    const uint32_t* on = reinterpret_cast<const uint32_t*>(bi->img.data() + bi->stride * t);
    const float* ol = reinterpret_cast<const float*>(on + NE);
    uint32_t* nn = reinterpret_cast<uint32_t*>(bi->fix_img.data() + bi->stride * t);
    float* nl = reinterpret_cast<float*>(nn + NE);
    const double* c = hcov.data() + static_cast<size_t>(t) * NE;
    for (int lo = 1; lo < NE; lo <<= 1) {   // level [lo, 2 lo): slots by cover
      lvl.resize(lo);
      for (int i = 0; i < lo; ++i) lvl[i] = lo + i;
      std::stable_sort(lvl.begin(), lvl.end(), [c](int32_t x, int32_t y) { return c[x] > c[y]; });
      if (!spread || lo <= kCls) {
        for (int i = 0; i < lo; ++i) pi[lvl[i]] = lo + i;
        continue;
      }
      // more than 32 pairs: slot s lies in bank class s % 32 (32 pairs of 8 B
      // span the 64 banks).  Sequential numbering gives class k the ranks k,
      // k + 32, k + 64 ...: the hottest node of each block of 32.  Instead
      // each node, hottest first, takes the class with the least cover so far
      // that still has room, so the classes carry equal traffic
      double load[kCls] = {0};
      int used[kCls] = {0};
      for (int i = 0; i < lo; ++i) {
        int k = -1;
        for (int b = 0; b < kCls; ++b)
          if (used[b] < lo / kCls && (k < 0 || load[b] < load[k])) k = b;
        pi[lvl[i]] = lo + k + kCls * used[k];
        load[k] += c[lvl[i]];
        ++used[k];
      }
    }
    auto relabel = [&](uint32_t w, int h) { return (w & ~0x7F8u) | (static_cast<uint32_t>(pi[h]) << 3); };
    nn[1] = relabel(on[1], 1);
    for (int v = 1; v < NE; ++v)
      for (int s = 0; s < 2; ++s) {
        const int ch = 2 * v + s, nw = 2 * pi[v] + s;
        if (ch < NE) nn[nw] = relabel(on[ch], ch);
        else nl[nw - NE] = ol[ch - NE];
      }
  }
}

template <typename XT, typename ACC>
bool pack_bheap(const ti_forest_desc* d, int D, BinImage* out,
                std::vector<int32_t>* leaf_ids) {
  const int F = d->n_features;
  const int LW = d->leaf_width;
  const RankTables<XT> rt = collect_ranks<XT>(d, false);
  const size_t m_max = rt.m_max;
  if (m_max > 65533) return false;
  BinImage image;   // *out and *leaf_ids are written once the forest qualifies
  BinImage* const bi = &image;
  bi->b16 = m_max > 253 ? 1 : 0;
  const int P = bi->b16 ? 2 : 4;
  bi->words = (F + P - 1) / P;
  // 512: measured +5% over 256 at F = 28 (32 waves/CU); a power of two in
  // [64, 512], as pack_rexplicit (the lane part is OR-ed into the offset)
  int R = 64;
  while (R < 512 && 2 * R <= env_int("TI_BHEAP_ROWS", 512)) R *= 2;
  while (R > 64 && static_cast<int64_t>(bi->words) * R * 4 > static_cast<int64_t>(ti::kBNodeOffMask) + 1)
    R >>= 1;
  if (static_cast<int64_t>(bi->words) * R * 4 > static_cast<int64_t>(ti::kBNodeOffMask) + 1) return false;
  bi->rows = R;
  bi->L = rt.L;
  bi->kary = 0;
  if constexpr (sizeof(XT) == 4) {
    // bucket-first search in place of the 5-ary one unless it would be no
    // shorter (TI_BIN_BUCKETS=0: never; TI_KARY=0 still means Eytzinger)
    const bool kary = env_int("TI_KARY", 1) != 0;
    const bool bkt = kary && env_int("TI_BIN_BUCKETS", 1) != 0 &&
                     bucket_tables(rt, &bi->tbl, &bi->bkt_nb);
    if (!bkt && kary) kary_tables(rt, &bi->tbl, &bi->kary);
    if (!bkt && !kary) eytzinger_tables(rt, &bi->tbl);
  } else {
    eytzinger_tables(rt, &bi->tbl);
  }
  // 512-row tiles: the offset bits are 0, 1 and 11..14, and each node word
  // also carries its own heap index in bits 3..10 (the fixed-layout walk's
  // pair address; treeinfer_kernels.h, kBNodeOffMask512)
  const bool with_index = R == 512;
  bi->mask = with_index ? ti::kBNodeOffMask512 : ti::kBNodeOffMask;
  auto node_word = [&](int64_t g) -> uint32_t {
    const int f = d->feature[g];
    const uint32_t rank = rt.rank(f, d->threshold[g]);
    const uint32_t off = static_cast<uint32_t>((f / P) * R * 4 + (f % P) * (4 / P));
    uint32_t w = off | (rank << 16);
    if (d->flags[g] & TI_NODE_NAN_LEFT) w |= ti::kBNodeNanLeft;
    return w;
  };
  const int NE = 1 << D;
  bi->stride = static_cast<int64_t>(align16(sizeof(uint32_t) * NE + sizeof(ACC) * NE * LW));
  bi->img.assign(static_cast<size_t>(bi->stride) * d->n_trees, 0);
  if (leaf_ids) leaf_ids->assign(static_cast<size_t>(NE) * d->n_trees, 0);
  struct Item { int32_t node; int32_t heap; int32_t level; double cov; };
  std::vector<Item> st;
  // the fixed walk's permuted image (fix_permute): float32 view, 512-row
  // tiles, depth-8 records of float leaves, covers in the model
  const bool perm = sizeof(XT) == 4 && sizeof(ACC) == 4 && with_index && D == 8 && LW == 1 && d->cover &&
                    env_int("TI_FIX_PERM", 1) != 0;
  std::vector<double> hcov(perm ? static_cast<size_t>(NE) * d->n_trees : 0, 0.0);
  for (int t = 0; t < d->n_trees; ++t) {
    unsigned char* rec = bi->img.data() + static_cast<size_t>(bi->stride) * t;
    uint32_t* nodes = reinterpret_cast<uint32_t*>(rec);
    ACC* leaves = reinterpret_cast<ACC*>(rec + sizeof(uint32_t) * NE);
    const int64_t b = d->tree_offset[t];
    st.assign(1, Item{0, 1, 0, d->cover ? d->cover[b] : 0.0});
    while (!st.empty()) {
      const Item it = st.back();
      st.pop_back();
      const int64_t g = b + it.node;
      if (perm && it.level < D) hcov[static_cast<size_t>(t) * NE + it.heap] = it.cov;
      if (it.level == D) {
        const int slot = it.heap - NE;
        for (int k = 0; k < LW; ++k)
          leaves[static_cast<size_t>(slot) * LW + k] = static_cast<ACC>(d->leaf_value[g * LW + k]);
        if (leaf_ids) (*leaf_ids)[static_cast<size_t>(t) * NE + slot] = d->leaf_id[g];
        continue;
      }
      const uint32_t idx = with_index ? static_cast<uint32_t>(it.heap) << 3 : 0u;
      if (d->feature[g] < 0) {   // shallow leaf: always-left padding down to level D
        nodes[it.heap] = (0xFFFFu << 16) | idx;
        st.push_back(Item{it.node, 2 * it.heap, it.level + 1, it.cov});
        st.push_back(Item{it.node, 2 * it.heap + 1, it.level + 1, 0.0});
      } else {
        nodes[it.heap] = node_word(g) | idx;
        st.push_back(Item{d->left[g], 2 * it.heap, it.level + 1,
                          d->cover ? d->cover[b + d->left[g]] : 0.0});
        st.push_back(Item{d->right[g], 2 * it.heap + 1, it.level + 1,
                          d->cover ? d->cover[b + d->right[g]] : 0.0});
      }
    }
  }
  if (perm) fix_permute(bi, hcov, NE, env_int("TI_FIX_SPREAD", 1) != 0);
  *out = std::move(image);
  return true;
}

// ------------------------------------------------ record explicit packing
// The record family is planned beside the forest: RecSlots is what every
// candidate shares, RecCandidate what one candidate packed and planned.  The
// planners below write a candidate only once nothing can fail any more, and
// choose_layout commits the one it keeps (commit_records).
struct RecSlots {
  std::vector<uint32_t> slot_of;   // descriptor node -> slot in its tree
  std::vector<uint32_t> rx_base, rx_nint;   // rx_base: [T+1]
  int64_t rx_slots = 0;
};
struct RecCandidate : RecArrays {
  int64_t lx_stage_cap = 0;   // stages of whole trees (7, 9)
  int32_t lx_ilp = 8;
  int32_t hx_top = 0, hx_stage = 0, hx_ilp = 8;   // heap tops (8, 9)
  int32_t tx8 = 0;   // layout 9's bottom
  uint32_t tx16_mask = 0;
};

// Slots of layout 6 (treeinfer_kernels.h, rx_walk): per tree the internal
// nodes breadth-first in [0, nint), then the leaves in the same breadth-first
// order as pack_explicit numbers them (so leaf ids / vector leaves share its
// tables), n slots for n nodes.  Returns false when a tree has more than
// 65,535 nodes (16-bit child slots).
bool plan_rx_slots(const ti_forest_desc* d, RecSlots* out) {
  std::vector<int32_t> level, next;
  RecSlots s;
  std::vector<uint32_t>* const slot_of = &s.slot_of;
  slot_of->assign(d->n_nodes, 0);
  s.rx_base.assign(d->n_trees + 1, 0);   // [T]: the slot count (staged layout)
  s.rx_nint.assign(d->n_trees, 0);
  if (d->n_nodes >= (int64_t(1) << 31)) return false;
  std::vector<int32_t> q;
  for (int t = 0; t < d->n_trees; ++t) {
    const int64_t b = d->tree_offset[t];
    const int64_t n = d->tree_offset[t + 1] - b;
    if (n > 65535) return false;
    s.rx_base[t] = static_cast<uint32_t>(b);   // a tree takes as many slots as nodes
    // level by level (the lockstep walks gather one level per step), and
    // within a level the internal nodes of largest cover first (cover_order)
    level.assign(1, 0);
    uint32_t n_int = 0;
    while (!level.empty()) {
      cover_order(d, b, &level);
      next.clear();
      for (const int32_t v : level) {
        const int64_t g = b + v;
        if (d->feature[g] < 0) continue;
        (*slot_of)[g] = n_int++;
        next.push_back(d->left[g]);
        next.push_back(d->right[g]);
      }
      level.swap(next);
    }
    // leaves in pack_explicit's numbering (leaf ids and vector leaves are
    // found as leaf_base + slot - nint): leaf_order
    leaf_order(d, b, &q);
    for (size_t i = 0; i < q.size(); ++i) (*slot_of)[b + q[i]] = n_int + static_cast<uint32_t>(i);
    s.rx_nint[t] = n_int;
  }
  s.rx_base[d->n_trees] = static_cast<uint32_t>(d->n_nodes);
  s.rx_slots = d->n_nodes;
  *out = std::move(s);
  return true;
}

// Records of one input view (ranks differ between the float32 and float64
// views).  Returns false when the bins do not fit u16 (more than 65,533
// distinct thresholds on a feature; 16,382 for zero-missing forests, whose
// bins are doubled) or, with b8, u8 (254; 126 with the zero rule: NaN is bin
// 0, values 1 .. m + 1), or the bin image does not fit 64 KB at 64-row tiles.
// u8 images hold four bins a word, so a tile of twice the rows (512,
// TI_RX_ROWS8) fits the LDS a u16 tile of 256 takes: 4 waves per SIMD
// instead of 2 at C3's 100 features.
template <typename XT, typename ACC>
bool pack_rexplicit(const ti_forest_desc* d, const ti_forest* f,
                    const std::vector<uint32_t>& slot_of, RecExplicit* out, bool b8) {
  const bool zero = f->zero_rule != 0;
  const RankTables<XT> rt = collect_ranks<XT>(d, zero);
  if (rt.m_max > (b8 ? (zero ? 126u : 254u) : (zero ? 16382u : 65533u))) return false;
  RecExplicit view;   // *out is written once the forest qualifies
  RecExplicit* const rx = &view;
  const int P = b8 ? 4 : 2;   // bins per word
  rx->b8 = b8 ? 1 : 0;
  rx->words = (d->n_features + P - 1) / P;
  const uint32_t nan_left = b8 ? ti::RxBins<true>::kNanLeft : ti::kRxNanLeft;
  const uint32_t zero_flip = b8 ? ti::RxBins<true>::kZeroFlip : ti::kRxZeroFlip;
  // a power of two in [64, 512]: the kernels OR the lane part (tid * 4) into
  // the feature's word offset (word * R * 4), which holds only then
  int R = 64;
  const int want_rows = b8 ? env_int("TI_RX_ROWS8", 512) : env_int("TI_RX_ROWS", 256);
  while (R < 512 && 2 * R <= want_rows) R *= 2;
  while (R > 64 && static_cast<size_t>(rx->words) * R * 4 > kFeatLdsMax) R >>= 1;
  if (static_cast<size_t>(rx->words) * R * 4 > kFeatLdsMax) return false;
  rx->rows = R;
  rx->L = rt.L;
  rx->kary = 0;
  // 5-ary tables for both views (float64: TI_KARY64, 32-byte nodes)
  if (env_int(sizeof(XT) == 4 ? "TI_KARY" : "TI_KARY64", 1) != 0) kary_tables(rt, &rx->tbl, &rx->kary);
  else eytzinger_tables(rt, &rx->tbl);
  // an even slot count: the staged layout copies whole 16-byte words
  rx->recs.assign(d->n_nodes + (d->n_nodes & 1), uint2{0u, 0u});
  const bool scalar_leaves = d->leaf_width == 1;
  for (int t = 0; t < d->n_trees; ++t) {
    const int64_t b = d->tree_offset[t];
    for (int64_t g = b; g < d->tree_offset[t + 1]; ++g) {
      uint2 r{0u, 0u};
      if (d->feature[g] < 0) {
        if (scalar_leaves) {
          const ACC v = static_cast<ACC>(d->leaf_value[g]);
          std::memcpy(&r, &v, sizeof(ACC));
        }
      } else {
        const int fe = d->feature[g];
        const uint32_t off = static_cast<uint32_t>((fe / P) * R * 4 + (fe % P) * (4 / P));
        const uint32_t rank = rt.rank(fe, d->threshold[g]);
        r.x = off | ((d->flags[g] & TI_NODE_NAN_LEFT) ? nan_left : 0u);
        if (zero) {
          r.x |= (2u * rank + 1u) << 16;   // <= 32,765: bit 31 stays clear
          if (d->flags[g] & TI_NODE_ZERO_FLIP) r.x |= zero_flip;
        } else {
          r.x |= rank << 16;
        }
        r.y = (slot_of[b + d->right[g]] << 16) | slot_of[b + d->left[g]];
      }
      rx->recs[b + slot_of[g]] = r;
    }
  }
  *out = std::move(view);
  return true;
}

// Staged record layout (7): forests whose trees are small enough that a run
// of several consecutive trees' records fits in LDS beside the bin image walk
// from LDS instead of gathering every node through the vector memory pipe
// (the bound of layout 6: TD busy 92 % of the kernel, profiles/r2_c3_l6b_*).
// The stage area is what 160 KB / TI_LX_WGS (2) workgroups per CU leave after
// the bin image, capped by the prefetch registers (kLxPf x 16 B per thread).
// A stage is a maximal run of consecutive trees whose records (their span
// widened to 16-byte words) fit the area.  Returns false (layout 6 stays) when
// fewer than two of the largest trees fit.
constexpr int kLxPf = 8;
// every masked bin address ((x & 0xFFFA) | lane offset <= 66,558) must stay
// inside the workgroup's LDS allocation: leaf records hold values, not offsets
constexpr size_t kLxMinLds = 66560;
// LDS bytes of the stage area of layouts 7 and 9 for tiles of R rows (the
// rule above: the bin image's remainder of a workgroup's share, within the
// prefetch registers, in whole 16-byte words)
size_t lx_stage_area(const RecArrays& c, int R) {
  const size_t bins = align16(static_cast<size_t>(std::max(c.rx[0].words, c.rx[1].words)) * R * 4 + 4);
  const int wgs = std::max(1, env_int("TI_LX_WGS", 2));
  size_t cap = kLdsPerCu / static_cast<size_t>(wgs);
  cap = cap > bins ? cap - bins : 0;
  return std::min(cap, static_cast<size_t>(kLxPf) * 16 * R) & ~size_t(15);
}
bool plan_lx_stages(const RecSlots& s, RecCandidate* c, int T) {
  const int R = c->rx[0].rows;
  if (c->rx[1].rows != R) return false;
  const size_t cap = lx_stage_area(*c, R);
  const std::vector<uint32_t>& b = s.rx_base;
  auto span = [&](int t0, int t1) {
    return ((static_cast<size_t>(b[t1]) * 8 + 15) & ~size_t(15)) - ((static_cast<size_t>(b[t0]) * 8) & ~size_t(15));
  };
  size_t biggest = 0;
  for (int t = 0; t < T; ++t) biggest = std::max(biggest, span(t, t + 1));
  if (T < 2 || cap < 2 * biggest + 16) return false;
  c->lx_stage.assign(1, 0);
  int t0 = 0;
  while (t0 < T) {
    int t1 = t0 + 1;
    while (t1 < T && span(t0, t1 + 1) <= cap) ++t1;
    c->lx_stage.push_back(t1);
    t0 = t1;
  }
  c->lx_stage_cap = static_cast<int64_t>(cap);
  // children as byte offsets in the tree (a stage is <= 32 KB: < 8,192 slots)
  for (auto& rx : c->rx)
    for (int t = 0; t < T; ++t)
      for (uint32_t v = b[t]; v < b[t] + s.rx_nint[t]; ++v) {
        uint2& r = rx.recs[v];
        r.y = (((r.y >> 16) << 3) << 16) | ((r.y & 0xFFFFu) << 3);
      }
  // trees in lockstep per lane: a stage's worth when stages hold 7 or 8 trees
  // (C3: 7 trees of 4,072 B per 30.7 KB stage; a group wider than the stage
  // walks a duplicate tree), else 4
  const double per_stage = static_cast<double>(T) / static_cast<double>(c->lx_stage.size() - 1);
  c->lx_ilp = per_stage >= 7.5 ? 8 : per_stage >= 6.5 ? 7 : 4;
  const int force_ilp = env_int("TI_LX_ILP", 0);
  if (force_ilp > 0) c->lx_ilp = force_ilp >= 8 ? 8 : force_ilp == 7 ? 7 : 4;
  return true;
}

// Heap tops of layout 8 (treeinfer_kernels.h, hexplicit_predict_kernel): per
// tree 2^(D0+1) u32 entries -- [0] unused, [1, 2^D0) the x words of layout
// 6's records at the heap positions of the top D0 levels (padding below a
// shallow leaf: rank 0xFFFF, NaN-left, which goes left on every bin), then at
// [2^D0, 2^(D0+1)) the layout-6 slot where the walk continues: the node at
// depth D0, or the leaf that ended the path above it.
constexpr uint32_t kHxPad = 0xFFFF0000u | ti::kRxNanLeft;
constexpr uint32_t kHxPad8 = 0xFFFF0000u | ti::RxBins<true>::kNanLeft;   // u8 bins (layout 9)
constexpr int kHxPf = 8;   // = PF of hexplicit_predict_kernel
void pack_htop(const ti_forest_desc* d, const std::vector<uint32_t>& slot_of, int D0,
               RecExplicit* rx) {
  const size_t NE = size_t(1) << D0;
  rx->top.assign(static_cast<size_t>(d->n_trees) * 2 * NE, 0u);
  struct Item { int32_t v; uint32_t p; int l; };
  std::vector<Item> st;
  for (int t = 0; t < d->n_trees; ++t) {
    const int64_t b = d->tree_offset[t];
    uint32_t* top = &rx->top[static_cast<size_t>(t) * 2 * NE];
    st.assign(1, Item{0, 1u, 0});
    while (!st.empty()) {
      const Item it = st.back();
      st.pop_back();
      const int64_t g = b + it.v;
      if (it.l == D0) {
        top[it.p] = slot_of[g];
        continue;
      }
      const bool leaf = d->feature[g] < 0;
      top[it.p] = leaf ? kHxPad : rx->recs[b + slot_of[g]].x;
      st.push_back(Item{leaf ? it.v : d->left[g], 2 * it.p, it.l + 1});
      st.push_back(Item{leaf ? it.v : d->right[g], 2 * it.p + 1, it.l + 1});
    }
  }
}

// Layout 8's parameters and images: the top depth D0 (TI_HX_TOP, default 8,
// at most the forest depth), ILP trees per lane (TI_HX_ILP: 4 or 8) and the
// stage (TI_HX_STAGE trees, default ILP; at most what the prefetch registers
// carry and what leaves the bin image room in 160 KB).  Falls back to layout 6
// (returns false) when even ILP tops do not fit.
constexpr int kHxMinDepth = 12;
// layout 8's top depth for a forest of depth D (TI_HX_TOP, default 8)
int hx_top_depth(int D) {
  return std::max(1, std::min(env_int("TI_HX_TOP", 8), std::min(D, 12)));
}
bool plan_htop(const ti_forest_desc* d, const RecSlots& s, RecCandidate* c, int D) {
  const int D0 = hx_top_depth(D);
  const int ilp = env_int("TI_HX_ILP", 8) >= 8 ? 8 : 4;
  const int R = c->rx[0].rows;
  if (c->rx[1].rows != R) return false;
  const size_t stride = static_cast<size_t>(8) << D0;
  const size_t bins = align16(static_cast<size_t>(std::max(c->rx[0].words, c->rx[1].words)) * R * 4 + 4);
  const size_t cap = std::min(static_cast<size_t>(kHxPf) * 16 * R, kLdsPerCu > bins ? kLdsPerCu - bins : 0);
  int S = env_int("TI_HX_STAGE", ilp);
  S = std::max(1, std::min<int>(S, d->n_trees));
  while (S > 1 && S * stride > cap) --S;
  if (S * stride > cap || S < std::min(ilp, d->n_trees)) return false;
  for (auto& rx : c->rx) pack_htop(d, s.slot_of, D0, &rx);
  c->hx_top = D0;
  c->hx_ilp = ilp;
  c->hx_stage = S;
  return true;
}

// Layout 9 (treeinfer_kernels.h, texplicit_predict_kernel): per tree, a heap
// top of D0 levels (as layout 8's, the entries at [2^D0, 2^(D0+1)) holding
// byte offsets into the bottom) and the bottom: layout 6's records from the
// first internal node at depth >= D0 on (breadth-first order puts the top's
// internal nodes first), children rebased to byte offsets from the bottom's
// start, padded to 16 bytes.  Stages as layout 7's.  Returns false (the
// caller keeps its choice) when two of the largest trees do not fit a stage
// or a bottom exceeds 16-bit byte offsets.
bool plan_tx(const ti_forest_desc* d, const RecSlots& s, RecCandidate* c, int D) {
  const std::vector<uint32_t>& slot_of = s.slot_of;
  int D0 = env_int("TI_TX_TOP", 6);
  D0 = std::max(1, std::min(D0, std::min(D, 10)));
  const int T = d->n_trees;
  const size_t NE = size_t(1) << D0;
  const uint32_t topb = static_cast<uint32_t>(8 * NE);
  std::vector<int32_t> dep, q;
  std::vector<uint32_t> ntop(T), nslots(T);
  std::vector<uint32_t> o(T + 1, 0), nint(T, 0);   // tree byte offsets, bottom internal counts
  for (int t = 0; t < T; ++t) {
    const int64_t b = d->tree_offset[t];
    const int32_t n = static_cast<int32_t>(d->tree_offset[t + 1] - b);
    dep.assign(n, 0);
    q.assign(1, 0);
    uint32_t nt = 0;
    for (size_t qi = 0; qi < q.size(); ++qi) {
      const int32_t v = q[qi];
      const int64_t g = b + v;
      if (d->feature[g] < 0) continue;
      if (dep[v] < D0) ++nt;
      dep[d->left[g]] = dep[d->right[g]] = dep[v] + 1;
      q.push_back(d->left[g]);
      q.push_back(d->right[g]);
    }
    ntop[t] = nt;
    nslots[t] = static_cast<uint32_t>(n) - nt;
    if (static_cast<size_t>(nslots[t]) * 8 > 65528) return false;
    nint[t] = s.rx_nint[t] - nt;
    const uint64_t end = o[t] + topb + ((static_cast<uint64_t>(nslots[t]) * 8 + 15) & ~uint64_t(15));
    if (end > 0xFFFFFFF0ull) return false;
    o[t + 1] = static_cast<uint32_t>(end);
  }
  // stages: as plan_lx_stages
  const int R = c->rx[0].rows;
  if (c->rx[1].rows != R) return false;
  const size_t cap = lx_stage_area(*c, R);
  size_t biggest = 0;
  for (int t = 0; t < T; ++t) biggest = std::max<size_t>(biggest, o[t + 1] - o[t]);
  if (T < 2 || cap < 2 * biggest) return false;
  // TI_LX_ILP > 0 also cuts stages to whole groups of that many trees
  // (plan_tx8 always does; here the default ILP follows the stage size)
  const int force_ilp = env_int("TI_LX_ILP", 0);
  const int cut = force_ilp > 0 ? (force_ilp >= 8 ? 8 : force_ilp == 7 ? 7 : 4) : 0;
  std::vector<int32_t> stages(1, 0);
  int t0 = 0;
  while (t0 < T) {
    int t1 = t0 + 1;
    while (t1 < T && o[t1 + 1] - o[t0] <= cap) ++t1;
    if (cut && t1 < T && t1 - t0 > cut) t1 = t0 + ((t1 - t0) / cut) * cut;
    stages.push_back(t1);
    t0 = t1;
  }
  // images: one per input view (the x words carry that view's ranks)
  for (auto& rx : c->rx) {
    rx.top.assign(o[T] / 4, 0u);
    struct Item { int32_t v; uint32_t p; int l; };
    std::vector<Item> st;
    for (int t = 0; t < T; ++t) {
      const int64_t b = d->tree_offset[t];
      const uint32_t nt = ntop[t];
      uint32_t* top = &rx.top[o[t] / 4];
      uint2* bot = reinterpret_cast<uint2*>(top + 2 * NE);
      st.assign(1, Item{0, 1u, 0});
      while (!st.empty()) {
        const Item it = st.back();
        st.pop_back();
        const int64_t g = b + it.v;
        if (it.l == D0) {
          top[it.p] = (slot_of[g] - nt) * 8u;
          continue;
        }
        const bool leaf = d->feature[g] < 0;
        top[it.p] = leaf ? (rx.b8 ? kHxPad8 : kHxPad) : rx.recs[b + slot_of[g]].x;
        st.push_back(Item{leaf ? it.v : d->left[g], 2 * it.p, it.l + 1});
        st.push_back(Item{leaf ? it.v : d->right[g], 2 * it.p + 1, it.l + 1});
      }
      // a leaf that ends a path above depth D0 is entered through the top:
      // its bottom entries were set by the walk above (slot_of - nt)
      for (uint32_t v = nt; v < nt + nslots[t]; ++v) {
        uint2 r = rx.recs[b + v];
        if (v < s.rx_nint[t]) {
          const uint32_t lft = (r.y & 0xFFFFu) - nt, rgt = (r.y >> 16) - nt;
          r.y = ((rgt * 8u) << 16) | (lft * 8u);
        }
        bot[v - nt] = r;
      }
    }
  }
  const double per_stage = static_cast<double>(T) / static_cast<double>(stages.size() - 1);
  c->lx_ilp = cut ? cut : per_stage >= 7.5 ? 8 : per_stage >= 6.5 ? 7 : 4;
  c->lx_stage = std::move(stages);
  c->lx_stage_cap = static_cast<int64_t>(cap);
  c->tx_off = std::move(o);
  c->tx_nint = std::move(nint);
  c->hx_top = D0;
  return true;
}

// Layout 9 with a compact bottom (u8 bins only; treeinfer_kernels.h,
// t8explicit_predict_kernel).  A bottom node is one u32 -- the u8 record x
// word (bin offset | flags | rank << 16) with byte 3 holding a pair index
// k' -- and a node's children sit side by side at positions 2k', 2k' + 1, so
// a step reads the bin and the children's 8-byte pair at once (one LDS round
// trip, the bytes of layout 9's one record read) and selects the child.
// Positions: the entries (nodes at depth D0 and leaves above it, in the
// order the top reaches them) first, padded to an even count, then the
// children of the bottom's internal nodes in breadth-first order (internal
// node k's at n_entries + 2k), so k' = n_entries / 2 + k < 256 for trees of
// <= 255 leaves.  A leaf loops on itself: x = kLeaf | rank 0xFF (even
// position: never right, NaN-left) or rank 0 (odd: always right), bin offset
// 0, k' = p / 2; its value and ordinal are read by position from global
// tables when the group is walked.  Returns false (u8 layout 9 keeps its
// records) when a tree has more than 255 leaves or the images do not fit.
//
// The u16 form (b16, plan_tx16; t16explicit_predict_kernel) keeps the u16
// record x word's rank (high half), word index, half-word bit and NaN-left
// (low half, lane part cleared) and puts k' into bits 2-9 of the lane part;
// a leaf is rank 0xFFFF (even) / 0 (odd) with bin offset 0, and no internal
// node may have either rank (the leaf test).  It needs tiles of >= 256 rows
// (bits 2-9 inside the lane part).  Zero-missing forests lose the word's zero-flip
// bit: a 64-byte table of one bit per position sits between the top and the
// bottom (kT16ZfBytes), read only by the slow step.
bool plan_tx8(const ti_forest_desc* d, const ti_forest* f, const RecSlots& s, RecCandidate* c, int D,
              bool b16) {
  const std::vector<uint32_t>& slot_of = s.slot_of;
  if (!b16 && (env_int("TI_TX8", 1) == 0 || !c->rx[0].b8 || !c->rx[1].b8)) return false;
  uint32_t bmask16 = 0, wmask16 = 0;
  if (b16) {
    if (env_int("TI_TX16", 1) == 0 || c->rx[0].b8 || c->rx[1].b8) return false;
    const int R = c->rx[0].rows;
    if (c->rx[1].rows != R || R < 256 || (R & (R - 1))) return false;
    int lg = 0;
    while ((1 << lg) < R) ++lg;
    wmask16 = (0xFFFFu << (2 + lg)) & 0xFFFFu;   // the word index bits
    bmask16 = wmask16 | 2u;
  }
  const uint32_t zfb = (b16 && f->zero_rule) ? ti::kT16ZfBytes : 0u;
  int D0 = env_int("TI_TX_TOP", b16 ? 8 : 6);
  // (the u16 bottom also runs without a top: D0 = 0, the root the only entry)
  D0 = std::max(b16 ? 0 : 1, std::min(D0, std::min(D, 10)));
  const int T = d->n_trees;
  const size_t NE = size_t(1) << D0;
  const uint32_t topb = static_cast<uint32_t>(8 * NE);
  const size_t acc_sz = f->accum == TI_F64 ? 8 : 4;
  // per tree: entries (the top's cut, left to right), then BFS children
  std::vector<std::vector<int32_t>> order(T);   // node at each bottom position (-1: pad)
  std::vector<std::vector<uint32_t>> kpair(T);  // per node: its children's pair index (internal)
  std::vector<uint32_t> pos(T + 1, 0), off(T + 1, 0);
  std::vector<int32_t> dep;
  struct Item { int32_t v; int l; };
  std::vector<Item> st;
  std::vector<int32_t> lvl, nxt;
  for (int t = 0; t < T; ++t) {
    const int64_t b = d->tree_offset[t];
    const int32_t n = static_cast<int32_t>(d->tree_offset[t + 1] - b);
    if (static_cast<int64_t>(n) > 509) return false;   // > 255 leaves
    std::vector<int32_t>& ord = order[t];
    ord.clear();
    // the top's cut in left-to-right order: depth-D0 nodes and shallow leaves
    st.assign(1, Item{0, 0});
    while (!st.empty()) {
      const Item it = st.back();
      st.pop_back();
      const int64_t g = b + it.v;
      if (it.l == D0 || d->feature[g] < 0) {
        ord.push_back(it.v);
        continue;
      }
      st.push_back(Item{d->right[g], it.l + 1});
      st.push_back(Item{d->left[g], it.l + 1});
    }
    const size_t n_entries = ord.size();
    if (n_entries & 1) ord.push_back(-1);
    const uint32_t half = static_cast<uint32_t>(ord.size() / 2);
    kpair[t].assign(n, 0u);
    uint32_t k = 0;
    // breadth-first over the bottom, a level at a time, each level's internal
    // nodes by cover (their children pairs: hot pairs first, cover_order)
    lvl.clear();
    for (const int32_t v : ord)
      if (v >= 0 && d->feature[b + v] >= 0) lvl.push_back(v);
    while (!lvl.empty()) {
      cover_order(d, b, &lvl);
      nxt.clear();
      for (const int32_t v : lvl) {
        if (half + k > 255) return false;
        kpair[t][v] = half + k++;
        for (const int32_t c : {d->left[b + v], d->right[b + v]}) {
          ord.push_back(c);
          if (d->feature[b + c] >= 0) nxt.push_back(c);
        }
      }
      lvl.swap(nxt);
    }
    pos[t + 1] = pos[t] + static_cast<uint32_t>(ord.size());
    const uint64_t bytes = topb + zfb + ((static_cast<uint64_t>(ord.size()) * 4 + 15) & ~uint64_t(15));
    if (bytes > 65520 || off[t] + bytes > 0xFFFFFFF0ull) return false;
    off[t + 1] = off[t] + static_cast<uint32_t>(bytes);
  }
  // stages: as plan_tx
  const int R = c->rx[0].rows;
  if (c->rx[1].rows != R) return false;
  const size_t cap = lx_stage_area(*c, R);
  size_t biggest = 0;
  for (int t = 0; t < T; ++t) biggest = std::max<size_t>(biggest, off[t + 1] - off[t]);
  if (T < 2 || cap < 2 * biggest) return false;
  // trees walked at once per lane: 4 (TI_LX_ILP overrides).  A stage holds a
  // whole number of ILP groups where it can (a group wider than the rest of
  // its stage walks duplicate trees): on c3_maxbin at 12 trees a stage, ILP 4
  // 4.70 ms, 7 5.29, 8 5.72 (profiles/r3_tx8_sweep.jsonl)
  const int force_ilp = env_int("TI_LX_ILP", 0);
  int ilp = force_ilp > 0 ? (force_ilp >= 8 ? 8 : force_ilp == 7 ? 7 : 4) : 4;
  // round 6: the u16 bottom two lanes a row when the tile's
  // 2R threads fit a workgroup of 512 and leaves are scalars (the lower lane
  // adds both halves' values in tree order); a group is 8 trees, 4 a lane.
  // TI_TX16_SPLIT=0 (developer knob) keeps the one-lane walk.
  const bool split = b16 && 2 * c->rx[0].rows <= 512 && d->leaf_width == 1 &&
                     env_int("TI_TX16_SPLIT", 1) != 0;
  if (b16) {   // the u16 kernel is instantiated at 4 and 8 trees a lane
    // (C3 at 1M rows, profiles/r5f_c3_t16_sweep.jsonl: 8 trees a lane and a
    // top of 8 levels 5.25-5.28 ms; 12 or 16 a lane 5.37-10.9 ms)
    ilp = split ? 8 : env_int("TI_TX16_ILP", 8) >= 8 ? 8 : 4;
  }
  std::vector<int32_t> stages(1, 0);
  int t0 = 0;
  while (t0 < T) {
    int t1 = t0 + 1;
    while (t1 < T && off[t1 + 1] - off[t0] <= cap) ++t1;
    if (t1 < T && t1 - t0 > ilp) {
      t1 = t0 + ((t1 - t0) / ilp) * ilp;
    }
    stages.push_back(t1);
    t0 = t1;
  }
  // position tables (shared by the views): leaf value and ordinal
  std::vector<unsigned char> val(static_cast<size_t>(pos[T]) * acc_sz, 0);
  std::vector<int32_t> ordinal(pos[T], 0);
  for (int t = 0; t < T; ++t) {
    const int64_t b = d->tree_offset[t];
    for (uint32_t p = 0; p < pos[t + 1] - pos[t]; ++p) {
      const int32_t v = order[t][p];
      if (v < 0 || d->feature[b + v] >= 0) continue;
      const size_t at = pos[t] + p;
      ordinal[at] = static_cast<int32_t>(slot_of[b + v] - s.rx_nint[t]);
      if (acc_sz == 8) {
        const double x = d->leaf_value[(b + v) * d->leaf_width];
        std::memcpy(&val[at * 8], &x, 8);
      } else {
        const float x = static_cast<float>(d->leaf_value[(b + v) * d->leaf_width]);
        std::memcpy(&val[at * 4], &x, 4);
      }
    }
  }
  // images per view
  constexpr uint32_t kLeaf = ti::RxBins<true>::kLeaf, kNanLeft = ti::RxBins<true>::kNanLeft;
  std::vector<int32_t> entry_of;
  std::vector<uint32_t> tops[2];   // moved into the views once both are built
  for (int i = 0; i < 2; ++i) {
    const RecExplicit& rx = c->rx[i];
    tops[i].assign(off[T] / 4, 0u);
    for (int t = 0; t < T; ++t) {
      const int64_t b = d->tree_offset[t];
      const int32_t n = static_cast<int32_t>(d->tree_offset[t + 1] - b);
      uint32_t* top = &tops[i][off[t] / 4];
      unsigned char* zf = reinterpret_cast<unsigned char*>(top + 2 * NE);
      uint32_t* bot = top + 2 * NE + zfb / 4;
      const std::vector<int32_t>& ord = order[t];
      entry_of.assign(n, -1);
      // a leaf word at position p: self-looping (even: rank 0xFF / 0xFFFF,
      // NaN-left; odd: rank 0), its own pair index
      auto leaf_word = [&](uint32_t p) {
        if (b16) return (p & 1 ? 0u : (0xFFFF0000u | 1u)) | ((p >> 1) << 2);
        return kLeaf | (p & 1 ? 0u : (0xFF0000u | kNanLeft)) | ((p >> 1) << 24);
      };
      for (uint32_t p = 0; p < ord.size(); ++p) {
        const int32_t v = ord[p];
        if (v < 0) {
          bot[p] = leaf_word(p);
          continue;
        }
        if (entry_of[v] < 0) entry_of[v] = static_cast<int32_t>(p);
        const int64_t g = b + v;
        if (d->feature[g] < 0) {
          bot[p] = leaf_word(p);
        } else if (b16) {
          const uint32_t xw = rx.recs[b + slot_of[g]].x;
          const uint32_t rk = xw >> 16;
          if (rk == 0u || rk == 0xFFFFu) return false;   // the ranks that mark a leaf
          bot[p] = (xw & (0xFFFF0000u | wmask16 | 3u)) | (kpair[t][v] << 2);
          if (zfb && (xw & ti::kRxZeroFlip)) zf[p >> 3] |= static_cast<unsigned char>(1u << (p & 7));
        } else {
          bot[p] = rx.recs[b + slot_of[g]].x | (kpair[t][v] << 24);
        }
      }
      // the top: x words, and at depth D0 the entry position
      struct TItem { int32_t v; uint32_t hp; int l; };
      std::vector<TItem> ts(1, TItem{0, 1u, 0});
      while (!ts.empty()) {
        const TItem it = ts.back();
        ts.pop_back();
        const int64_t g = b + it.v;
        if (it.l == D0) {
          top[it.hp] = static_cast<uint32_t>(entry_of[it.v]);
          continue;
        }
        const bool leaf = d->feature[g] < 0;
        top[it.hp] = leaf ? (b16 ? kHxPad : kHxPad8) : rx.recs[b + slot_of[g]].x;
        ts.push_back(TItem{leaf ? it.v : d->left[g], 2 * it.hp, it.l + 1});
        ts.push_back(TItem{leaf ? it.v : d->right[g], 2 * it.hp + 1, it.l + 1});
      }
    }
  }
  for (int i = 0; i < 2; ++i) c->rx[i].top = std::move(tops[i]);
  c->tx_off = std::move(off);
  c->tx8_pos = std::move(pos);
  c->tx8_val = std::move(val);
  c->tx8_ord = std::move(ordinal);
  c->tx_nint.assign(T, 0);
  c->lx_stage = std::move(stages);
  c->lx_stage_cap = static_cast<int64_t>(cap);
  c->lx_ilp = ilp;
  c->hx_top = D0;
  c->tx8 = split ? 3 : b16 ? 2 : 1;
  c->tx16_mask = bmask16;
  return true;
}

// Mean depth of the leaves of a forest (every leaf counted once).
double mean_leaf_depth(const ti_forest_desc* d) {
  double sum = 0;
  int64_t n_leaf = 0;
  std::vector<int32_t> dep, q;
  for (int t = 0; t < d->n_trees; ++t) {
    const int64_t b = d->tree_offset[t];
    const int32_t n = static_cast<int32_t>(d->tree_offset[t + 1] - b);
    dep.assign(n, 0);
    q.assign(1, 0);   // breadth-first: a parent's depth is set first
    for (size_t qi = 0; qi < q.size(); ++qi) {
      const int32_t v = q[qi];
      const int64_t g = b + v;
      if (d->feature[g] < 0) {
        sum += dep[v];
        ++n_leaf;
      } else {
        dep[d->left[g]] = dep[d->right[g]] = dep[v] + 1;
        q.push_back(d->left[g]);
        q.push_back(d->right[g]);
      }
    }
  }
  return n_leaf ? sum / n_leaf : 0.0;
}

// The stage-size rule of the heap layouts and the binned heap: from S trees,
// grow by `step` (the trees a lane walks at once) while the workgroups-per-CU
// count of the first size holds -- occupancy is what hides the LDS latency of
// the walk (measured: 3 WG/CU beat 2 WG/CU by 1.7x at F = 28) -- within `cap`
// (the prefetch registers) and the forest.  `fixed`: the LDS bytes before the
// stage; area(n): those of a stage of n trees.
template <typename Area>
int64_t grow_stage(int64_t S, int64_t step, int64_t cap, int64_t T, size_t fixed, Area area) {
  auto wgs = [&](int64_t n) { return kLdsPerCu / (fixed + area(n)); };
  const size_t best = S >= 1 ? wgs(S) : 0;
  while (S + step <= cap && S + step <= T && wgs(S + step) >= best) S += step;
  return S;
}

// Stage size S (trees) of the heap layouts (0, 10) for tiles of R rows: the
// smallest useful stage (kTilp trees, fewer if LDS is short) grown by
// grow_stage, capped by the prefetch registers (kPf x 16 B x R).  `fixed`:
// feature image + NaN flag word.  TI_HEAP_LDS_KB overrides with a fixed
// per-workgroup budget.  0: not even one record fits.
int64_t heap_stage_trees(const ti_forest* f, int64_t stride_b, size_t fixed, int R) {
  const int64_t cap = static_cast<int64_t>(ti::kPf) * 16 * R / stride_b;
  static const int budget_kb = env_int("TI_HEAP_LDS_KB", 0);
  int64_t S;
  if (budget_kb > 0) {
    const size_t b = static_cast<size_t>(budget_kb) * 1024;
    S = b > fixed ? static_cast<int64_t>((b - fixed) / stride_b) : 0;
    if (S >= ti::kTilp) S -= S % ti::kTilp;
  } else {
    S = std::min<int64_t>(ti::kTilp, cap);
    while (S > 1 && fixed + static_cast<size_t>(S * stride_b) > kLdsPerCu) --S;
    S = grow_stage(S, ti::kTilp, cap, f->T, fixed,
                   [&](int64_t n) { return static_cast<size_t>(n * stride_b); });
  }
  if (S < 1 || fixed + static_cast<size_t>(S * stride_b) > kLdsPerCu) return 0;
  S = std::min<int64_t>(S, cap);
  S = std::min<int64_t>(S, f->T);
  return S;
}

// Layout 10 (treeinfer_cheap.h): whether the forest's records fit, and if so
// the packed images (in the heap layout's fields).  The float32 view (what
// XGBoost's DMatrix feeds) must stage at least as many trees as a lane walks
// at once (kTilp) within the kPf x 16 x R bytes of the prefetch registers --
// `forced` (TI_FORCE_LAYOUT=cheap) asks for one; the float64 view for one, so
// either input type runs.  Both need their feature image in LDS, and the
// categorical nodes one rule (the kernel is compiled per rule).
bool plan_cheap(const ti_forest_desc* desc, ti_forest* f, int D, bool forced) {
  if (f->has_cat_xgb && f->has_cat_lgb) return false;
  const size_t acc_sz = f->accum == TI_F64 ? 8 : 4;
  const int want_rows = env_int("TI_HEAP_ROWS", 0);
  const int r32 = pick_rows(f->F, 4, want_rows), r64 = pick_rows(f->F, 8, want_rows);
  if (r32 <= 0 || r64 <= 0 || r32 > 512 || r64 > 512) return false;
  if (static_cast<size_t>(f->F) * r32 * 4 > kFeatLdsMax || static_cast<size_t>(f->F) * r64 * 8 > kFeatLdsMax)
    return false;
  const uint32_t sc32 = static_cast<uint32_t>(r32) * 4u, sc64 = static_cast<uint32_t>(r64) * 8u;
  if (static_cast<uint64_t>(f->F) * std::max(sc32, sc64) > ti::kMetaFeatMask) return false;
  const int64_t s32 = cheap_stride<float>(desc, D, acc_sz), s64 = cheap_stride<double>(desc, D, acc_sz);
  const int64_t cap32 = static_cast<int64_t>(ti::kPf) * 16 * r32 / s32;
  if (cap32 < (forced ? 1 : ti::kTilp)) return false;
  const size_t fixed32 = align16(static_cast<size_t>(f->F) * r32 * 4) + 16;
  const size_t fixed64 = align16(static_cast<size_t>(f->F) * r64 * 8) + 16;
  if (heap_stage_trees(f, s32, fixed32, r32) < 1 || heap_stage_trees(f, s64, fixed64, r64) < 1)
    return false;
  f->rows32 = r32;
  f->rows64 = r64;
  f->stride32 = s32;
  f->stride64 = s64;
  HostImage& h = *f->host;
  for_views(f->accum, [&](auto x, auto acc, int i) {
    pack_cheap<decltype(x), decltype(acc)>(desc, D, i ? s64 : s32, i ? sc64 : sc32,
                                           i ? &h.heap64 : &h.heap32,
                                           i ? nullptr : &h.heap_leaf_ids);
    return true;
  });
  return true;
}

// Linear leaves: a record per (tree, library leaf id) -- what TI_OUTPUT_LEAF
// reports is what pass 2 indexes -- and the terms as 16-byte records.
int pack_linear(const ti_forest_desc* d, HostImage* h) {
  h->lin_leaf_base.assign(d->n_trees, 0);
  h->lin_terms.resize(static_cast<size_t>(d->n_lin_terms));
  for (int64_t i = 0; i < d->n_lin_terms; ++i) {
    ti::LinTerm& t = h->lin_terms[i];
    t.coeff = d->lin_coeff[i];
    t.feature = static_cast<uint32_t>(d->lin_feature[i]);
    t.pad = 0;
  }
  std::vector<char> seen;
  for (int t = 0; t < d->n_trees; ++t) {
    const int64_t b = d->tree_offset[t], e = d->tree_offset[t + 1];
    int64_t nl = 0;
    for (int64_t g = b; g < e; ++g) nl += d->feature[g] < 0;
    const size_t base = h->lin_leaves.size();
    h->lin_leaf_base[t] = static_cast<int64_t>(base);
    h->lin_leaves.resize(base + static_cast<size_t>(nl));
    seen.assign(static_cast<size_t>(nl), 0);
    for (int64_t g = b; g < e; ++g) {
      if (d->feature[g] >= 0) continue;
      const int64_t id = d->leaf_id[g];
      if (id < 0 || id >= nl || seen[id])
        return fail(TI_ERR_INVALID, "linear leaves need leaf_id = 0 .. L-1 within tree " +
                                        std::to_string(t));
      seen[id] = 1;
      ti::LinLeaf& l = h->lin_leaves[base + static_cast<size_t>(id)];
      l.lconst = d->lin_const[g];
      l.fallback = d->leaf_value[g];
      l.begin = static_cast<uint32_t>(d->lin_offset[g]);
      l.count = static_cast<uint32_t>(d->lin_offset[g + 1] - d->lin_offset[g]);
      l.pad[0] = l.pad[1] = 0;
    }
  }
  return TI_OK;
}

// The record family's choice becomes the forest's: plan scalars into the
// forest, arrays into its host image (moved, not copied).
void commit_records(ti_forest* f, RecSlots&& s, RecCandidate&& c) {
  HostImage& h = *f->host;
  for (int i = 0; i < 2; ++i) f->rx[i] = c.rx[i];   // the RecPlan part
  f->rx_slots = s.rx_slots;
  f->n_stages = c.lx_stage.empty() ? 0 : static_cast<int32_t>(c.lx_stage.size() - 1);
  f->lx_stage_cap = c.lx_stage_cap;
  f->lx_ilp = c.lx_ilp;
  f->hx_top = c.hx_top;
  f->hx_stage = c.hx_stage;
  f->hx_ilp = c.hx_ilp;
  f->tx8 = c.tx8;
  f->tx16_mask = c.tx16_mask;
  h.rx_base = std::move(s.rx_base);
  h.rx_nint = std::move(s.rx_nint);
  h.rec = std::move(static_cast<RecArrays&>(c));
}

// The layout of a forest whose model fields are filled, with its plan scalars
// and host image.  Candidates are tried in a fixed order; one that does not
// take the forest leaves nothing behind, and f->layout is assigned here, once.
//
// Binned heap for depth <= 8, the record layouts (6-9) for deeper trees;
// categorical splits: the categorical heap (10) for XGBoost-rule forests of
// depth <= 8 whose records fit a stage (plan_cheap), the float explicit kernel
// (1) otherwise and for every LightGBM-rule forest;
// TI_FORCE_LAYOUT=heap|explicit|rexplicit|lexplicit|hexplicit|texplicit|cheap
// overrides (tests run every layout on the same forest); cheap puts any
// categorical forest of depth <= 8 on layout 10, whichever rule it uses.
int choose_layout(const ti_forest_desc* desc, ti_forest* f) {
  HostImage& h = *f->host;
  const size_t acc_sz = f->accum == TI_F64 ? 8 : 4;
  const int D = f->depth;
  h.group.assign(f->T, 0);   // every layout's kernels read the tree groups
  if (f->LW == 1)
    for (int t = 0; t < f->T; ++t) h.group[t] = desc->tree_group[t];
  const char* force = env_knob("TI_FORCE_LAYOUT");
  const std::string want = force ? force : "";
  bool use_heap = D <= kMaxHeapDepth;
  if (want == "heap" && D <= kMaxHeapDepth) use_heap = true;
  if (want == "explicit" || want == "rexplicit" || want == "lexplicit" || want == "hexplicit" ||
      want == "texplicit")
    use_heap = false;
  // categorical splits are evaluated by the explicit kernel and the categorical heap
  if (f->has_cat) use_heap = false;
  bool use_cheap = false;
  if (f->has_cat && D >= 1 && D <= kMaxHeapDepth &&
      (want == "cheap" || (f->has_cat_xgb && want.empty())))
    use_cheap = plan_cheap(desc, f, D, want == "cheap");
  // binned heap (rank-binned features, 4-byte nodes) for complete-able trees
  // without LightGBM zero-missing or categorical splits; TI_FORCE_LAYOUT=heap
  // keeps the float-compare heap kernel
  bool use_bheap = use_heap && want != "heap" && f->zero_rule == 0 && D >= 1;
  if (use_bheap) {
    BinImage bh[2];
    std::vector<int32_t> leaf_ids;
    use_bheap = for_views(f->accum, [&](auto x, auto acc, int i) {
      return pack_bheap<decltype(x), decltype(acc)>(desc, D, &bh[i], i ? nullptr : &leaf_ids);
    });
    if (use_bheap) {
      for (int i = 0; i < 2; ++i) {
        f->bh[i] = bh[i];   // the BinPlan part
        h.bh[i] = std::move(bh[i]);
      }
      h.heap_leaf_ids = std::move(leaf_ids);
    }
  }
  Layout chosen;
  if (use_cheap) {
    chosen = kLayoutCatHeap;   // packed by plan_cheap
  } else if (use_bheap) {
    chosen = kLayoutBinHeap;
  } else if (use_heap) {
    const int NI = (1 << D) - 1, NL = 1 << D;
    chosen = kLayoutHeap;
    const int64_t s32 = static_cast<int64_t>(align16(sizeof(HeapNode<float>) * NI + acc_sz * NL * f->LW));
    const int64_t s64 = static_cast<int64_t>(align16(sizeof(HeapNode<double>) * NI + acc_sz * NL * f->LW));
    const int want_rows = env_int("TI_HEAP_ROWS", 0);
    const int r32 = pick_rows(f->F, 4, want_rows), r64 = pick_rows(f->F, 8, want_rows);
    // feature byte offset: column of the [F][R] LDS image, or of the row in HBM
    const uint32_t sc32 = r32 ? static_cast<uint32_t>(r32) * 4u : 4u;
    const uint32_t sc64 = r64 ? static_cast<uint32_t>(r64) * 8u : 8u;
    if (static_cast<uint64_t>(f->F) * std::max(sc32, sc64) > ti::kMetaFeatMask)
      return fail(TI_ERR_UNSUPPORTED, "feature image offsets exceed 24 bits");
    f->stride32 = s32;
    f->stride64 = s64;
    f->rows32 = r32;
    f->rows64 = r64;
    for_views(f->accum, [&](auto x, auto acc, int i) {
      pack_heap<decltype(x), decltype(acc)>(desc, D, i ? s64 : s32, i ? sc64 : sc32,
                                            i ? &h.heap64 : &h.heap32,
                                            i ? nullptr : &h.heap_leaf_ids);
      return true;
    });
  } else {
    chosen = kLayoutExplicit;
    with_acc(f->accum, [&](auto acc) {
      pack_explicit<decltype(acc)>(desc, &h);
      return true;
    });
    // record explicit slots (layout 6) unless a categorical split needs raw
    // values or another explicit kernel is forced
    RecSlots slots;
    bool rx_ok = !f->has_cat && want != "explicit" && plan_rx_slots(desc, &slots);
    RecCandidate c;
    auto pack_views = [&](bool b8) {
      c = RecCandidate();
      return for_views(f->accum, [&](auto x, auto acc, int i) {
        return pack_rexplicit<decltype(x), decltype(acc)>(desc, f, slots.slot_of, &c.rx[i], b8);
      });
    };
    // u8 bins where every feature's thresholds fit them and layout 9 takes
    // the forest (only layout 9 reads u8 images; TI_RX_B8=0 keeps u16)
    const bool try8 = rx_ok && env_int("TI_RX_B8", 1) != 0 &&
                      (want.empty() || want == "texplicit");
    const bool b8 = try8 && pack_views(true) &&
                    (plan_tx8(desc, f, slots, &c, D, false) || plan_tx(desc, slots, &c, D));
    if (!b8 && rx_ok) rx_ok = pack_views(false);
    if (rx_ok) {
      chosen = kLayoutRecord;
      // trees in flight per lane: 16 for shallow-on-average forests (C3,
      // mean leaf depth ~9: 7.70 ms vs 7.79 at 8), 8 for deep ones (C4,
      // sklearn depth 16: 3.06 ms vs 3.13 at 16); profiles/r2_rx_sweep.jsonl
      const double md = mean_leaf_depth(desc);
      f->rx_ilp = md < 12.0 ? 16 : 8;
      const int force_ilp = env_int("TI_RX_ILP", 0);
      if (force_ilp > 0) f->rx_ilp = force_ilp >= 16 ? 16 : force_ilp >= 8 ? 8 : 4;
      // small trees: a heap top and the rest staged in LDS (layout 9; C3
      // 1M rows 5.83 vs 6.15 ms for layout 7), or all records staged
      // (layout 7, forced, or when layout 9 does not fit); deep trees too large for a
      // stage: heap tops in LDS, the rest gathered (layout 8)
      const bool auto_ok = want != "rexplicit" && want != "hexplicit" && want != "lexplicit";
      if (b8) {
        chosen = kLayoutTopStaged;   // u8 bins (planned above)
      } else if ((want == "texplicit" || auto_ok) &&
                 (plan_tx8(desc, f, slots, &c, D, true) || plan_tx(desc, slots, &c, D))) {
        chosen = kLayoutTopStaged;   // the compact u16 bottom where it fits, else records
      } else if ((want == "lexplicit" || auto_ok) && plan_lx_stages(slots, &c, f->T)) {
        chosen = kLayoutStaged;
      } else if ((want == "hexplicit" || (want != "rexplicit" && D >= kHxMinDepth)) &&
                 plan_htop(desc, slots, &c, D)) {
        chosen = kLayoutHeapTop;
      }
      commit_records(f, std::move(slots), std::move(c));
    }
  }
  f->layout = chosen;
  return TI_OK;
}

}  // namespace
