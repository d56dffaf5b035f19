// treeinfer_shap_interv.h -- interventional TreeSHAP against a background set
// (TI_OUTPUT_CONTRIB_INTERV): the mask, contribution and finishing kernels,
// ti_forest_set_background's host side (set_background) and launch_interv.
// Included by treeinfer.hip alone, after treeinfer_shap.h, whose path tables
// (ShapPath, ShapElem, the category sets) it reads as they are.
//
// For a request row x and a background row z, take a leaf path with elements
// e_0 .. e_{n-1} and the bitmasks ox / oz of the elements x / z satisfy.  A
// hybrid of x and z reaches the leaf only if ox | oz is all ones.  With
// U = ox & ~oz, V = oz & ~ox, a = |U|, b = |V| the leaf value v adds
//   + v (a-1)! b! / (a+b)!  to each feature of U,
//   - v a! (b-1)! / (a+b)!  to each feature of V,
// nothing to the elements both satisfy (a = b = 0: the bias alone).  phi is
// the mean over z.  Zero fractions (ShapElem.zf) are never read.
#pragma once

#include "treeinfer_shap.h"

constexpr int kIntervMaxN = 32;                       // longest path, in unique features
constexpr int kIntervTabN = kIntervMaxN + 1;
constexpr uint64_t kIntervMaskBytesMax = 1ull << 30;  // mask table of one replica
constexpr uint64_t kIntervPartBytesMax = 256ull << 20;   // partials of one row block
constexpr int64_t kIntervMaskPathsPerBlock = 256;

// w[a][b] = (a-1)! b! / (a+b)! = 1 / (a C(a+b, b)), a >= 1; row 0 is zero.
// Filled on the host by the recurrence w[a][0] = 1/a, w[a][b] = w[a][b-1] b /
// (a+b): at most 2 x 32 roundings from the exact value.
struct IntervWeights {
  double v[kIntervTabN * kIntervTabN];
};
inline IntervWeights make_interv_weights() {
  IntervWeights t;
  for (int b = 0; b < kIntervTabN; ++b) t.v[b] = 0.0;
  for (int a = 1; a < kIntervTabN; ++a) {
    t.v[a * kIntervTabN] = 1.0 / a;
    for (int b = 1; b < kIntervTabN; ++b)
      t.v[a * kIntervTabN + b] = t.v[a * kIntervTabN + b - 1] * b / (double)(a + b);
  }
  return t;
}

// The background mask table [n_paths][B] (u32, bit i = z follows element i):
// one lane per z row, a block of paths per blockIdx.y, so a wave's 64 writes
// of one path are one line.  Elements come through uniform loads.
template <typename XT>
__global__ void __launch_bounds__(64) interv_masks_kernel(
    const XT* __restrict__ Z, int64_t B, int64_t stride, int32_t cols, int32_t zero_map_on,
    const ShapPath* __restrict__ paths, int64_t n_paths, const ShapElem* __restrict__ elems,
    const ShapCatRef* __restrict__ cat_refs, const uint32_t* __restrict__ cat_words,
    int64_t paths_per_block, uint32_t* __restrict__ masks) {
  const int64_t z = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = z < B;
  const XT* zr = Z + (live ? z : B - 1) * stride;
  const int64_t p_begin = (int64_t)blockIdx.y * paths_per_block;
  const int64_t p_end = p_begin + paths_per_block < n_paths ? p_begin + paths_per_block : n_paths;
  for (int64_t p = p_begin; p < p_end; ++p) {
    const ShapPath P = paths[p];
    const ShapElem* pe = elems + P.first;
    uint32_t oz = 0u;
    for (int i = 0; i < P.n; ++i) {
      const ShapElem e = pe[i];
      double x = e.feature < cols ? (double)zr[e.feature] : __builtin_nan("");
      if (zero_map_on && __builtin_fabs(x) <= (double)1e-35f) x = 0.0;
      oz |= (shap_follow(e, x, P.first + i, cat_refs, cat_words) ? 1u : 0u) << i;
    }
    if (live) masks[p * B + z] = oz;
  }
}

// One 64-lane workgroup per (request row blockIdx.x, 64-row z block
// blockIdx.y, path slice blockIdx.z); a lane owns one background row.  Per
// path the header and elements are uniform loads; lane i < n tests x against
// element i and a ballot gives ox for the whole wave; a lane then reads its oz
// (one coalesced dword), forms U and V, fetches the two weights from the LDS
// copy of the weight table (stride tw = maxl + 1) and adds the signed terms
// times the leaf value(s) to its own accumulators phi[j * 64] in LDS.  Which
// elements can be in U (x follows) and which in V (x does not) is uniform, so
// an element costs one LDS read-modify-write.  At the end the 64 lanes of a
// column are summed in a fixed order (column j starts at lane j % 64: no two
// lanes of the wave read one bank) and the W sums go to
// part[((row * ZB + zb) * slices + slice) * W + j].  Tail lanes of the last z
// block add zero.  Float64 throughout.
template <typename XT, int MAXN>
__global__ void __launch_bounds__(64) interv_contrib_kernel(
    const XT* __restrict__ X, int64_t stride, int32_t cols, int32_t zero_map_on,
    const ShapPath* __restrict__ paths, int64_t n_paths, const ShapElem* __restrict__ elems,
    const double* __restrict__ leafv, int32_t LW, int32_t K, int32_t F, int32_t maxl,
    const ShapCatRef* __restrict__ cat_refs, const uint32_t* __restrict__ cat_words,
    const uint32_t* __restrict__ masks, int64_t B, const double* __restrict__ weights,
    int64_t paths_per_slice, double* __restrict__ part) {
  extern __shared__ double shap_lds[];
  const int lane = threadIdx.x;
  const int W = K * (F + 1);
  const int tw = maxl + 1;
  double* phi = shap_lds + lane;          // phi[j * 64]
  double* wt = shap_lds + (size_t)W * 64;  // [tw][tw]
  for (int j = 0; j < W; ++j) phi[j * 64] = 0.0;
  for (int i = lane; i < tw * tw; i += 64) wt[i] = weights[(i / tw) * kIntervTabN + (i % tw)];
  __syncthreads();
  const XT* xr = X + (int64_t)blockIdx.x * stride;
  const int64_t z = (int64_t)blockIdx.y * 64 + lane;
  const bool zlive = z < B;
  const uint32_t* mz = masks + (zlive ? z : B - 1);
  const int64_t p_begin = (int64_t)blockIdx.z * paths_per_slice;
  const int64_t p_end = p_begin + paths_per_slice < n_paths ? p_begin + paths_per_slice : n_paths;
  for (int64_t p = p_begin; p < p_end; ++p) {
    const ShapPath P = paths[p];
    const int n = P.n;
    const ShapElem* pe = elems + P.first;
    const uint32_t oz = mz[p * B];
    bool fx = false;
    if (lane < n) {
      const ShapElem e = pe[lane];
      double x = e.feature < cols ? (double)xr[e.feature] : __builtin_nan("");
      if (zero_map_on && __builtin_fabs(x) <= (double)1e-35f) x = 0.0;
      fx = shap_follow(e, x, P.first + lane, cat_refs, cat_words);
    }
    const uint32_t ox = static_cast<uint32_t>(__ballot(fx));
    const uint32_t full = n >= 32 ? ~0u : (1u << n) - 1u;
    const uint32_t U = ox & ~oz, V = oz & ~ox & full;
    const bool hit = zlive && ((ox | oz) & full) == full && (U | V) != 0u;
    if (!__any(hit)) continue;   // no z of the block has a term on this path
    const int a = __popc(U), b = __popc(V);
    // row 0 of the table is zero: a == 0 gives no U term, b == 0 no V term
    const double wu = hit ? wt[a * tw + b] : 0.0;
    const double wv = hit ? -wt[b * tw + a] : 0.0;
    const double* lv = leafv + P.leaf * LW;
    if (LW == 1) {
      const double l0 = lv[0];
      double* pg = phi + (size_t)P.group * (F + 1) * 64;
#pragma unroll
      for (int i = 0; i < MAXN; ++i) {
        if (i < n) {
          const bool xin = ((ox >> i) & 1u) != 0u;   // uniform
          const bool zin = ((oz >> i) & 1u) != 0u;
          const double c = xin ? (zin ? 0.0 : wu) : (zin ? wv : 0.0);
          pg[pe[i].feature * 64] += c * l0;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < MAXN; ++i) {
        if (i < n) {
          const bool xin = ((ox >> i) & 1u) != 0u;
          const bool zin = ((oz >> i) & 1u) != 0u;
          const double c = xin ? (zin ? 0.0 : wu) : (zin ? wv : 0.0);
          const int fe = pe[i].feature;
          for (int k = 0; k < LW; ++k) phi[(k * (F + 1) + fe) * 64] += c * lv[k];
        }
      }
    }
  }
  __syncthreads();
  double* pp = part + (((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z) * W;
  for (int j = lane; j < W; j += 64) {
    const double* col = shap_lds + (size_t)j * 64;
    double t = 0.0;
    for (int s = 0; s < 64; ++s) t += col[(s + j) & 63];
    pp[j] = t;
  }
}

// One thread per output element: the partials of its (row, column) summed in
// (z block, slice) order, over B and the divisor; the bias column is the
// background's mean margin.
template <typename ACC>
__global__ void __launch_bounds__(256) interv_finish_kernel(
    const double* __restrict__ part, int64_t rows, int32_t per_row, int32_t K, int32_t F,
    const double* __restrict__ bias, double B, double divisor, ACC* __restrict__ out) {
  const int W = K * (F + 1);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * W) return;
  const int64_t row = i / W;
  const int j = (int)(i - row * W);
  const int g = j / (F + 1);
  if (j - g * (F + 1) == F) {
    out[i] = (ACC)bias[g];
    return;
  }
  const double* pp = part + row * per_row * W + j;
  double t = 0.0;
  for (int q = 0; q < per_row; ++q) t += pp[(int64_t)q * W];
  out[i] = (ACC)(t / B / divisor);
}

namespace {

// the background of one replica (device current)
void free_interv(DeviceForest& d) {
  if (d.interv_masks) (void)hipFree(d.interv_masks);
  if (d.interv_bias) (void)hipFree(d.interv_bias);
  if (d.interv_weights) (void)hipFree(d.interv_weights);
  d.interv_masks = nullptr;
  d.interv_bias = nullptr;
  d.interv_weights = nullptr;
  d.bytes -= d.interv_bytes;
  d.interv_bytes = 0;
}

void clear_background(ti_forest* f) {
  int dev0 = 0;
  (void)hipGetDevice(&dev0);
  for (auto& dp : f->devs) {
    (void)hipSetDevice(dp->device);
    free_interv(*dp);
  }
  (void)hipSetDevice(dev0);
  f->interv_B = 0;
}

// What no background can change: the forest shapes TI_OUTPUT_CONTRIB_INTERV
// does not serve.  (A path of more than 32 features and the mask table's size
// are known only once the path tables exist: interv_paths, set_background.)
int interv_refusal(const ti_forest* f) {
  if (f->has_cat_xgb)
    return fail(TI_ERR_UNSUPPORTED,
                "interventional contributions of categorical splits with XGBoost's rule "
                "(TI_NODE_CAT_XGB) are not supported; categorical splits with LightGBM's rule are");
  if (f->linear)
    return fail(TI_ERR_UNSUPPORTED,
                "TI_OUTPUT_CONTRIB_INTERV of a forest with linear leaves (a leaf has no one value)");
  if (f->pre_steps > 0)
    return fail(TI_ERR_UNSUPPORTED,
                "TI_OUTPUT_CONTRIB_INTERV of a forest with pre-steps is not supported");
  const int64_t W = static_cast<int64_t>(f->K) * (f->F + 1);
  if (W > kShapLdsW)
    return fail(TI_ERR_UNSUPPORTED,
                "interventional contributions need n_groups * (n_features + 1) <= " +
                    std::to_string(kShapLdsW) + " (a row's accumulators in LDS); the forest has " +
                    std::to_string(W));
  return TI_OK;
}

// The path tables (ensure_shap) and the path-length limit.
int interv_paths(ti_forest* f) {
  const int rc = ensure_shap(f);
  if (rc) return rc;
  if (f->shap_maxl > kIntervMaxN)
    return fail(TI_ERR_UNSUPPORTED,
                "interventional contributions need paths of at most 32 unique features; the "
                "forest's longest has " + std::to_string(f->shap_maxl));
  return TI_OK;
}

// ti_forest_set_background on one (unchunked) forest; bias [K] is the mean
// margin of Z.  Z goes to each replica for the run of interv_masks_kernel
// only: the kernels of a request read the masks, never Z.
int set_background(ti_forest* f, const void* Z, int zdt, int64_t B, int32_t cols, int64_t stride,
                   const std::vector<double>& bias) {
  int rc = interv_paths(f);
  if (rc) return rc;
  const int64_t n_paths = f->shap_npaths;
  const uint64_t mask_bytes = static_cast<uint64_t>(n_paths) * static_cast<uint64_t>(B) * 4;
  if (mask_bytes > kIntervMaskBytesMax || (B + 63) / 64 > 65535)
    return fail(TI_ERR_UNSUPPORTED,
                "the background mask table (" + std::to_string(n_paths) + " paths x " +
                    std::to_string(B) + " rows x 4 B) exceeds 1 GiB per device");
  static const IntervWeights weights = make_interv_weights();
  const size_t zs = zdt == TI_F64 ? 8 : 4;
  const size_t z_bytes = static_cast<size_t>((B - 1) * stride + cols) * zs;
  int dev0 = 0;
  TI_HIP(hipGetDevice(&dev0));
  for (auto& dp : f->devs) {
    DeviceForest& d = *dp;
    if ((rc = fail_hip(hipSetDevice(d.device), "hipSetDevice"))) break;
    void* dz = nullptr;
    bool ok = hipMalloc(&dz, z_bytes) == hipSuccess &&
              hipMalloc(reinterpret_cast<void**>(&d.interv_masks), std::max<uint64_t>(mask_bytes, 4)) == hipSuccess &&
              hipMalloc(reinterpret_cast<void**>(&d.interv_bias), bias.size() * 8) == hipSuccess &&
              hipMalloc(reinterpret_cast<void**>(&d.interv_weights), sizeof(weights)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      if (dz) (void)hipFree(dz);
      rc = fail(TI_ERR_NOMEM, "background allocation failed");
      break;
    }
    d.interv_bytes = static_cast<int64_t>(mask_bytes + bias.size() * 8 + sizeof(weights));
    d.bytes += d.interv_bytes;
    hipError_t e = hipMemcpy(dz, Z, z_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.interv_bias, bias.data(), bias.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.interv_weights, weights.v, sizeof(weights), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_paths > 0) {
      const dim3 grid(static_cast<unsigned>((B + 63) / 64),
                      static_cast<unsigned>((n_paths + kIntervMaskPathsPerBlock - 1) / kIntervMaskPathsPerBlock));
      if (zdt == TI_F32)
        hipLaunchKernelGGL((interv_masks_kernel<float>), grid, dim3(64), 0, d.stream,
                           static_cast<const float*>(dz), B, stride, cols, f->lgb_zero_map, d.shap_paths,
                           n_paths, d.shap_elems, d.shap_cat_refs, d.shap_cat_words,
                           kIntervMaskPathsPerBlock, d.interv_masks);
      else
        hipLaunchKernelGGL((interv_masks_kernel<double>), grid, dim3(64), 0, d.stream,
                           static_cast<const double*>(dz), B, stride, cols, f->lgb_zero_map, d.shap_paths,
                           n_paths, d.shap_elems, d.shap_cat_refs, d.shap_cat_words,
                           kIntervMaskPathsPerBlock, d.interv_masks);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    }
    (void)hipFree(dz);
    if ((rc = fail_hip(e, "background upload"))) break;
  }
  (void)hipSetDevice(dev0);
  if (rc) {
    const std::string err = g_last_error;
    clear_background(f);
    return fail(rc, err);
  }
  f->interv_B = B;
  return TI_OK;
}

// TI_OUTPUT_CONTRIB_INTERV on one (unchunked) forest.  Rows go in blocks whose
// partials [rows, z blocks, slices, W] stay within kIntervPartBytesMax; path
// slices are chosen as launch_contrib chooses them, with the (row, z block)
// pairs as the waves, so a one-row request still spreads over the device.  The
// partials live in the replica's grow-only call scratch (CallScratch: taken
// under its mutex, handed on behind interv_finish_kernel with its event).
int launch_interv(ti_forest* f, DeviceForest& d, const void* X, int xdt, int64_t rows,
                  int32_t cols, int64_t stride, void* out, hipStream_t stream) {
  int rc = interv_refusal(f);
  if (rc) return rc;
  if ((rc = interv_paths(f))) return rc;
  const int64_t B = f->interv_B;
  if (B <= 0 || !d.interv_masks)
    return fail(TI_ERR_INVALID,
                "TI_OUTPUT_CONTRIB_INTERV needs a background set (ti_forest_set_background)");
  if (rows == 0) return TI_OK;
  const int W = f->K * (f->F + 1);
  const int64_t n_paths = f->shap_npaths;
  const int64_t ZB = (B + 63) / 64;
  const int maxn = f->shap_maxl <= 8 ? 8 : f->shap_maxl <= 16 ? 16 : 32;
  const int tw = f->shap_maxl + 1;
  const size_t lds = (static_cast<size_t>(W) * 64 + static_cast<size_t>(tw) * tw) * 8;
  const int force_slices = env_int("TI_SHAP_SLICES", 0);
  const int64_t waves = std::max<int64_t>(rows, 1) * ZB;
  int64_t slices = force_slices > 0 ? force_slices : (kShapWaveTarget + waves - 1) / waves;
  if (force_slices <= 0)
    slices = std::min<int64_t>(slices, std::max<int64_t>(1, n_paths / kShapMinPathsPerSlice));
  slices = std::min<int64_t>(slices, kShapMaxSlices);
  slices = std::max<int64_t>(std::min<int64_t>(slices, std::max<int64_t>(n_paths, 1)), 1);
  const int64_t pps = (n_paths + slices - 1) / slices;
  const int64_t per_row = ZB * slices;
  const int64_t rb = std::max<int64_t>(
      1, std::min<int64_t>(rows, static_cast<int64_t>(kIntervPartBytesMax /
                                                       (static_cast<uint64_t>(per_row) * W * 8))));
  ScratchHold part_buf(d, stream);   // given back behind the last interv_finish_kernel
  if (!part_buf.take(static_cast<size_t>(rb * per_row * W) * 8))
    return fail(TI_ERR_NOMEM, "interventional partials allocation failed");
  double* part = static_cast<double*>(part_buf.p);
  const size_t xs = xdt == TI_F64 ? 8 : 4;
  const size_t as = f->accum == TI_F64 ? 8 : 4;
#define TI_INTERV(XT_, N_)                                                                        \
  do {                                                                                            \
    KernelFn fn_ = reinterpret_cast<KernelFn>(interv_contrib_kernel<XT_, N_>);                    \
    rc = ensure_lds_attr(d.device, fn_);                                                          \
    if (rc == TI_OK) {                                                                            \
      occ_note(fn_, 64, lds);                                                                     \
      hipLaunchKernelGGL((interv_contrib_kernel<XT_, N_>),                                        \
                         dim3((unsigned)n, (unsigned)ZB, (unsigned)slices), dim3(64), lds, stream, \
                         static_cast<const XT_*>(xb), stride, cols, f->lgb_zero_map, d.shap_paths, \
                         n_paths, d.shap_elems, d.shap_leaf, f->LW, f->K, f->F, f->shap_maxl,     \
                         d.shap_cat_refs, d.shap_cat_words, d.interv_masks, B, d.interv_weights,  \
                         pps, part);                                                              \
    }                                                                                             \
  } while (0)
#define TI_INTERV_N(XT_)                        \
  do {                                          \
    if (maxn == 8) TI_INTERV(XT_, 8);           \
    else if (maxn == 16) TI_INTERV(XT_, 16);    \
    else TI_INTERV(XT_, 32);                    \
  } while (0)
  for (int64_t r0 = 0; r0 < rows && rc == TI_OK; r0 += rb) {
    const int64_t n = std::min(rb, rows - r0);
    const void* xb = static_cast<const unsigned char*>(X) + static_cast<size_t>(r0 * stride) * xs;
    if (xdt == TI_F32) TI_INTERV_N(float);
    else TI_INTERV_N(double);
    if (rc) break;
    unsigned char* ob = static_cast<unsigned char*>(out) + static_cast<size_t>(r0) * W * as;
    const unsigned g2 = static_cast<unsigned>((n * W + 255) / 256);
    if (f->accum == TI_F64)
      hipLaunchKernelGGL((interv_finish_kernel<double>), dim3(g2), dim3(256), 0, stream, part, n,
                         (int32_t)per_row, f->K, f->F, d.interv_bias, (double)B, f->divisor,
                         reinterpret_cast<double*>(ob));
    else
      hipLaunchKernelGGL((interv_finish_kernel<float>), dim3(g2), dim3(256), 0, stream, part, n,
                         (int32_t)per_row, f->K, f->F, d.interv_bias, (double)B, f->divisor,
                         reinterpret_cast<float*>(ob));
  }
#undef TI_INTERV_N
#undef TI_INTERV
  if (rc == TI_OK && hipGetLastError() != hipSuccess)
    rc = fail(TI_ERR_DEVICE, "interventional contributions launch failed");
  return rc;
}

}  // namespace
