// treeinfer_shap.h -- TreeSHAP contributions (TI_OUTPUT_CONTRIB): the device
// kernels, the host path tables (ShapBuilder) with their lazy build and upload
// (ensure_shap, ensure_shap_table), and launch_contrib.  Included by
// treeinfer.hip alone.
#pragma once

#include "treeinfer_forest.h"


// Whether value x (the zero map applied) follows every split of a path
// element: the interval and the NaN / zero flags of its numerical splits
// (shap_follow_num) and, under kShapCat, membership of its category set
// (shap_follow_cat); shap_follow is both.  The element comes through scalar
// loads, so the flag test is a scalar branch; the set's {first, nwords} is one
// scalar load too and only the set's word is per lane.
__device__ __forceinline__ bool shap_follow_num(const ShapElem& e, double x) {
  if (x != x) return (e.flags & kShapNanOk) != 0;
  if (x == 0.0) return (e.flags & kShapZeroOk) != 0;
  return !(e.flags & kShapEmpty) && !(x <= e.lo) && x <= e.hi;   // lo NaN: unbounded below
}

// LightGBM's rule (ti::cat_left) against the element's set: codes are trunc(x)
// for x in (-1, 2^31); anything else, and a code past the set's last word,
// follows iff the path never turned left (kShapCatOutside).  The zero map
// cannot change the answer: |x| <= 1e-35 is code 0 either way.
__device__ __forceinline__ bool shap_follow_cat(uint32_t flags, double x, int64_t ei,
                                                const ShapCatRef* __restrict__ cat_refs,
                                                const uint32_t* __restrict__ cat_words) {
  // both fields in one load, ahead of the divergent part below
  const uint64_t rw = *reinterpret_cast<const uint64_t*>(cat_refs + ei);
  const ShapCatRef r{static_cast<uint32_t>(rw), static_cast<uint32_t>(rw >> 32)};
  const bool inside = x > -1.0 && x < 2147483648.0;
  const uint32_t v = inside ? static_cast<uint32_t>(x) : 0u;
  const bool covered = inside && (v >> 5) < r.nwords;
  const uint32_t word = covered ? cat_words[r.first + (v >> 5)] : 0u;
  return covered ? ((word >> (v & 31u)) & 1u) != 0u : (flags & kShapCatOutside) != 0;
}

__device__ __forceinline__ bool shap_follow(const ShapElem& e, double x, int64_t ei,
                                            const ShapCatRef* __restrict__ cat_refs,
                                            const uint32_t* __restrict__ cat_words) {
  bool follow = shap_follow_num(e, x);
  if (e.flags & kShapCat) follow = shap_follow_cat(e.flags, x, ei, cat_refs, cat_words) && follow;
  return follow;
}

// One row per lane (64-row blocks).  Per path: the one fractions of the
// row, then the path weights extended from scratch (ExtendPath) and, per
// element, the unwound sum (UnwoundPathSum) times (one - zero) times the
// leaf value, added to the element's feature.  Path weights and one
// fractions live in LDS as [index][lane].  acc is float64 [rows, K*(F+1)];
// the last pass divides by average_divisor, writes the bias and converts to
// ACC.
template <typename XT, typename ACC>
__global__ void __launch_bounds__(64) contrib_kernel(
    const XT* __restrict__ X, int64_t rows, int64_t stride, int32_t cols, int32_t zero_map_on,
    const ShapPath* __restrict__ paths, int64_t n_paths, const ShapElem* __restrict__ elems,
    const double* __restrict__ leafv, int32_t LW, int32_t K, int32_t F, int32_t maxl,
    const double* __restrict__ bias, double divisor, double* __restrict__ acc,
    ACC* __restrict__ out, const ShapCatRef* __restrict__ cat_refs,
    const uint32_t* __restrict__ cat_words) {
  extern __shared__ double shap_lds[];
  const int lane = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * 64 + lane;
  const bool live = row < rows;
  double* w = shap_lds;                         // [maxl + 1][64]
  double* ob = shap_lds + (size_t)(maxl + 1) * 64;   // [maxl][64]
  const XT* xr = X + (live ? row : rows - 1) * stride;
  const int W = K * (F + 1);
  double* ph = acc + (live ? row : 0) * W;
  for (int64_t p = 0; p < n_paths; ++p) {
    const ShapPath P = paths[p];
    const int n = P.n;
    for (int i = 0; i < n; ++i) {
      const ShapElem e = elems[P.first + i];
      double x = e.feature < cols ? (double)xr[e.feature] : __builtin_nan("");
      if (zero_map_on && __builtin_fabs(x) <= (double)1e-35f) x = 0.0;
      const bool follow = shap_follow(e, x, P.first + i, cat_refs, cat_words);
      ob[i * 64 + lane] = follow ? 1.0 : 0.0;
    }
    w[lane] = 1.0;
    for (int d = 1; d <= n; ++d) {
      const double zf = elems[P.first + d - 1].zf;
      const double of = ob[(d - 1) * 64 + lane];
      w[d * 64 + lane] = 0.0;
      for (int i = d - 1; i >= 0; --i) {
        w[(i + 1) * 64 + lane] += of * w[i * 64 + lane] * (i + 1) / (double)(d + 1);
        w[i * 64 + lane] = zf * w[i * 64 + lane] * (d - i) / (double)(d + 1);
      }
    }
    for (int e_i = 1; e_i <= n; ++e_i) {
      const ShapElem e = elems[P.first + e_i - 1];
      const double of = ob[(e_i - 1) * 64 + lane];
      const double zf = e.zf;
      double next = w[n * 64 + lane];
      double total = 0.0;
      for (int i = n - 1; i >= 0; --i) {
        if (of != 0.0) {
          const double tmp = next * (n + 1) / ((i + 1) * of);
          total += tmp;
          next = w[i * 64 + lane] - tmp * zf * (n - i) / (double)(n + 1);
        } else {
          total += (w[i * 64 + lane] / zf) / ((n - i) / (double)(n + 1));
        }
      }
      const double scale = total * (of - zf);
      if (live) {
        if (LW == 1) {
          ph[P.group * (F + 1) + e.feature] += scale * leafv[P.leaf];
        } else {
          for (int k = 0; k < LW; ++k) ph[k * (F + 1) + e.feature] += scale * leafv[P.leaf * LW + k];
        }
      }
    }
  }
  if (!live) return;
  ACC* o = out + row * W;
  for (int g = 0; g < K; ++g) {
    for (int f = 0; f < F; ++f) o[g * (F + 1) + f] = (ACC)(ph[g * (F + 1) + f] / divisor);
    o[g * (F + 1) + F] = (ACC)bias[g];
  }
}

// 1/k for k = 0..64 (entry 0 unused), exactly rounded at compile time.
template <int... I>
struct ShapInvTable {
  double v[sizeof...(I)];
};
template <int... I>
constexpr ShapInvTable<I...> make_inv(std::integer_sequence<int, I...>) {
  return {{(I == 0 ? 0.0 : 1.0 / I)...}};
}
__constant__ ShapInvTable kShapInv = make_inv(std::make_integer_sequence<int, 65>{});

// The contrib kernel with the path arithmetic in registers.  Everything about
// a path (its length, elements, zero fractions, leaf) is the same for all 64
// lanes, so it comes through scalar loads; a lane only owns its row's one
// fractions (a bitmask: they are 0 or 1) and its path weights w[0..n], which
// stay in VGPRs because every loop that indexes them is unrolled over MAXN.
// The divisions of contrib_kernel become products with compile-time ratios
// or the 1/k table.  The row's contributions accumulate in LDS [W][64]
// (W = K * (F + 1) <= kShapLdsW), so no global read-modify-write.
constexpr int kShapLdsW = 128;
constexpr int kShapTabStride = 8;   // coefficients per one-pattern in the table (paths of <= 8 elements)
constexpr int64_t kShapWaveTarget = 65536;        // 64-row waves per contrib launch (sweep: profiles/r1_shap_sweep.log)
constexpr int64_t kShapMinPathsPerSlice = 256;
constexpr int64_t kShapMaxSlices = 64;
constexpr uint64_t kShapPartBytesMax = 2ull << 30;
// The longest path, in MAXN, whose extend / unwind arithmetic a float32
// forest does in float32.  The unwound sums cancel, and the loss grows with
// the path: against the float64 reference, chains of 16 distinct features
// measured 3.7e-7 (contributions) and 9.4e-7 (interactions) of the row's
// scale, of 17 1.8e-6 and 1.9e-6, of 32 1.5e-2 and 4.3e-2, where float64
// arithmetic gives the float32 output's own rounding, 6e-8
// (profiles/shap_edge_error_before.jsonl; xgboost's own bst_float TreeShap loses
// 9e-3 on the same 32-element chains).  So the MAXN = 32 instantiations are
// float64 only.
constexpr int kShapF32MaxN = 16;
// TAB: the per-element coefficients UnwoundPathSum x (one - zero) of every
// path and every pattern of one fractions were computed once per forest
// (shap_table_kernel, the same expressions in the same MT arithmetic), so a
// path costs its n element tests, n coefficient loads at [path][om] and the
// n accumulations, instead of the O(n^2) extend and unwind: the same floats.
template <typename XT, typename ACC, typename MT, int MAXN, bool TAB = false>
__global__ void __launch_bounds__(64) contrib_reg_kernel(
    const XT* __restrict__ X, int64_t rows, int64_t stride, int32_t cols, int32_t zero_map_on,
    const ShapPath* __restrict__ paths, int64_t n_paths, const ShapElem* __restrict__ elems,
    const double* __restrict__ leafv, int32_t LW, int32_t K, int32_t F, int32_t maxl,
    const double* __restrict__ bias, double divisor, double* __restrict__ part,
    int64_t paths_per_slice, ACC* __restrict__ out, const MT* __restrict__ tab,
    const int64_t* __restrict__ tab_off, const ShapCatRef* __restrict__ cat_refs,
    const uint32_t* __restrict__ cat_words) {
  (void)maxl;
  extern __shared__ double shap_lds[];
  const int lane = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * 64 + lane;
  const bool live = row < rows;
  const XT* xr = X + (live ? row : rows - 1) * stride;
  const int W = K * (F + 1);
  MT* phi = reinterpret_cast<MT*>(shap_lds) + lane;   // phi[j * 64]
  for (int j = 0; j < W; ++j) phi[j * 64] = MT(0);
  const int64_t p_begin = (int64_t)blockIdx.y * paths_per_slice;
  const int64_t p_end = p_begin + paths_per_slice < n_paths ? p_begin + paths_per_slice : n_paths;
  for (int64_t p = p_begin; p < p_end; ++p) {
    const ShapPath P = paths[p];
    const int n = P.n;
    const ShapElem* pe = elems + P.first;
    uint32_t om = 0u;                             // one fractions, bit i = element i
    for (int i = 0; i < n; ++i) {
      const ShapElem e = pe[i];
      double x = e.feature < cols ? (double)xr[e.feature] : __builtin_nan("");
      if (zero_map_on && __builtin_fabs(x) <= (double)1e-35f) x = 0.0;
      om |= (shap_follow_num(e, x) ? 1u : 0u) << i;
    }
    if (cat_refs) {
      // A forest with categorical nodes (one scalar branch a path; the others
      // run the loop above alone): clear the bits of the elements whose
      // category set the row is not in.
      for (int i = 0; i < n; ++i) {
        const int32_t fe = pe[i].feature;
        const uint32_t fl = pe[i].flags;
        if (!(fl & kShapCat)) continue;
        const double x = fe < cols ? (double)xr[fe] : __builtin_nan("");
        if (!shap_follow_cat(fl, x, P.first + i, cat_refs, cat_words)) om &= ~(1u << i);
      }
    }
    if constexpr (TAB) {
      // the pattern's coefficients: kShapTabStride values, 32- or 64-byte
      // aligned, read with whole-vector loads (a lane touches one line)
      typedef MT v4_t __attribute__((ext_vector_type(4)));
      const v4_t* c4 = reinterpret_cast<const v4_t*>(tab + tab_off[p] + (int64_t)om * kShapTabStride);
      MT c[kShapTabStride];
#pragma unroll
      for (int j = 0; j < kShapTabStride / 4; ++j) {
        const v4_t v = c4[j];
        c[4 * j] = v.x;
        c[4 * j + 1] = v.y;
        c[4 * j + 2] = v.z;
        c[4 * j + 3] = v.w;
      }
      const double* lv = leafv + P.leaf * LW;
      if (LW == 1) {
        const MT l0 = static_cast<MT>(lv[0]);
#pragma unroll
        for (int e_i = 0; e_i < kShapTabStride; ++e_i)
          if (e_i < n) phi[(P.group * (F + 1) + pe[e_i].feature) * 64] += c[e_i] * l0;
      } else {
#pragma unroll
        for (int e_i = 0; e_i < kShapTabStride; ++e_i)
          if (e_i < n)
            for (int k = 0; k < LW; ++k)
              phi[(k * (F + 1) + pe[e_i].feature) * 64] += c[e_i] * static_cast<MT>(lv[k]);
      }
      continue;
    }
    // ExtendPath from scratch
    MT w[MAXN + 1];
    w[0] = MT(1);
#pragma unroll
    for (int d = 1; d <= MAXN; ++d) {
      if (d <= n) {
        const MT of = ((om >> (d - 1)) & 1u) ? MT(1) : MT(0);
        const MT zf = static_cast<MT>(pe[d - 1].zf);
        w[d] = MT(0);
#pragma unroll
        for (int i = d - 1; i >= 0; --i) {
          w[i + 1] += of * w[i] * static_cast<MT>((double)(i + 1) / (double)(d + 1));
          w[i] = zf * w[i] * static_cast<MT>((double)(d - i) / (double)(d + 1));
        }
      }
    }
    const MT rn1 = static_cast<MT>(n + 1);
    const MT in1 = static_cast<MT>(kShapInv.v[n + 1]);
    MT wn = MT(0);                              // w[n]
#pragma unroll
    for (int i = 0; i <= MAXN; ++i)
      if (i == n) wn = w[i];
    const double* lv = leafv + P.leaf * LW;
    // UnwoundPathSum per element, times (one - zero) times the leaf value
    if constexpr (std::is_same<MT, float>::value) {
      // Two elements at once in packed float32 (v_pk_mul/add_f32), both
      // branches of the unwind evaluated and selected per lane: the branch
      // on `one` diverges within a wave anyway.  Same per-element expression
      // order as the scalar loop below, so the same float results.
      typedef float f2 __attribute__((ext_vector_type(2)));
      for (int e_i = 0; e_i < n; e_i += 2) {
        const bool pair = e_i + 1 < n;
        const ShapElem ea = pe[e_i];
        const ShapElem eb = pe[pair ? e_i + 1 : e_i];
        const bool one_a = ((om >> e_i) & 1u) != 0u;
        const bool one_b = ((om >> (pair ? e_i + 1 : e_i)) & 1u) != 0u;
        const f2 zf = {static_cast<float>(ea.zf), static_cast<float>(eb.zf)};
        const f2 izf = f2{1.0f, 1.0f} / zf;
        f2 next = {wn, wn};
        f2 tot1 = {0.0f, 0.0f}, tot0 = {0.0f, 0.0f};
#pragma unroll
        for (int i = MAXN - 1; i >= 0; --i) {
          if (i < n) {
            const f2 tmp = next * (rn1 * static_cast<float>(1.0 / (double)(i + 1)));
            tot1 += tmp;
            next = w[i] - tmp * zf * (static_cast<float>(n - i) * in1);
            tot0 += w[i] * izf * (rn1 * static_cast<float>(kShapInv.v[n - i]));
          }
        }
        const float sa = (one_a ? tot1.x : tot0.x) * ((one_a ? 1.0f : 0.0f) - zf.x);
        const float sb = (one_b ? tot1.y : tot0.y) * ((one_b ? 1.0f : 0.0f) - zf.y);
        if (LW == 1) {
          const float l0 = static_cast<float>(lv[0]);
          phi[(P.group * (F + 1) + ea.feature) * 64] += sa * l0;
          if (pair) phi[(P.group * (F + 1) + eb.feature) * 64] += sb * l0;
        } else {
          for (int k = 0; k < LW; ++k) {
            const float lk = static_cast<float>(lv[k]);
            phi[(k * (F + 1) + ea.feature) * 64] += sa * lk;
            if (pair) phi[(k * (F + 1) + eb.feature) * 64] += sb * lk;
          }
        }
      }
      continue;
    }
    for (int e_i = 0; e_i < n; ++e_i) {
      const ShapElem e = pe[e_i];
      const bool one = ((om >> e_i) & 1u) != 0u;
      const MT zf = static_cast<MT>(e.zf);
      MT total = MT(0);
      if (one) {
        MT next = wn;
#pragma unroll
        for (int i = MAXN - 1; i >= 0; --i) {
          if (i < n) {
            const MT tmp = next * (rn1 * static_cast<MT>(1.0 / (double)(i + 1)));
            total += tmp;
            next = w[i] - tmp * zf * (static_cast<MT>(n - i) * in1);
          }
        }
      } else {
        const MT izf = MT(1) / zf;
#pragma unroll
        for (int i = MAXN - 1; i >= 0; --i) {
          if (i < n) total += w[i] * izf * (rn1 * static_cast<MT>(kShapInv.v[n - i]));
        }
      }
      const MT scale = total * ((one ? MT(1) : MT(0)) - zf);
      if (LW == 1) {
        phi[(P.group * (F + 1) + e.feature) * 64] += scale * static_cast<MT>(lv[0]);
      } else {
        for (int k = 0; k < LW; ++k)
          phi[(k * (F + 1) + e.feature) * 64] += scale * static_cast<MT>(lv[k]);
      }
    }
  }
  if (!live) return;
  if (part) {
    // path slice blockIdx.y: raw partial sums, [slice][W][rows] (coalesced)
    double* pp = part + (int64_t)blockIdx.y * W * rows + row;
    for (int j = 0; j < W; ++j) pp[(int64_t)j * rows] = static_cast<double>(phi[j * 64]);
    return;
  }
  ACC* o = out + row * W;
  for (int g = 0; g < K; ++g) {
    for (int f = 0; f < F; ++f)
      o[g * (F + 1) + f] = (ACC)(static_cast<double>(phi[(g * (F + 1) + f) * 64]) / divisor);
    o[g * (F + 1) + F] = (ACC)bias[g];
  }
}

// The coefficient table of contrib_reg_kernel<TAB>: one workgroup per path,
// a lane per pattern om of one fractions (bit i = element i followed): the
// path weights extended from scratch and, per element, UnwoundPathSum x
// (one - zero) -- the expressions of contrib_reg_kernel in the same order
// and type, so the table holds the floats the kernel would compute.
template <typename MT, int MAXN>
__global__ void __launch_bounds__(256) shap_table_kernel(const ShapPath* __restrict__ paths,
                                                         const ShapElem* __restrict__ elems,
                                                         const int64_t* __restrict__ tab_off,
                                                         MT* __restrict__ tab) {
  const ShapPath P = paths[blockIdx.x];
  const int n = P.n;
  const ShapElem* pe = elems + P.first;
  MT* out = tab + tab_off[blockIdx.x];
  for (uint32_t om = threadIdx.x; om < (1u << n); om += blockDim.x) {
    MT w[MAXN + 1];
    w[0] = MT(1);
#pragma unroll
    for (int d = 1; d <= MAXN; ++d) {
      if (d <= n) {
        const MT of = ((om >> (d - 1)) & 1u) ? MT(1) : MT(0);
        const MT zf = static_cast<MT>(pe[d - 1].zf);
        w[d] = MT(0);
#pragma unroll
        for (int i = d - 1; i >= 0; --i) {
          w[i + 1] += of * w[i] * static_cast<MT>((double)(i + 1) / (double)(d + 1));
          w[i] = zf * w[i] * static_cast<MT>((double)(d - i) / (double)(d + 1));
        }
      }
    }
    const MT rn1 = static_cast<MT>(n + 1);
    const MT in1 = static_cast<MT>(kShapInv.v[n + 1]);
    MT wn = MT(0);
#pragma unroll
    for (int i = 0; i <= MAXN; ++i)
      if (i == n) wn = w[i];
    for (int e_i = 0; e_i < n; ++e_i) {
      const bool one = ((om >> e_i) & 1u) != 0u;
      const MT zf = static_cast<MT>(pe[e_i].zf);
      MT total;
      if constexpr (std::is_same<MT, float>::value) {
        // contrib_reg_kernel's packed float path: both sums, then the select
        const float izf = 1.0f / zf;
        float next = wn, tot1 = 0.0f, tot0 = 0.0f;
#pragma unroll
        for (int i = MAXN - 1; i >= 0; --i) {
          if (i < n) {
            const float tmp = next * (rn1 * static_cast<float>(1.0 / (double)(i + 1)));
            tot1 += tmp;
            next = w[i] - tmp * zf * (static_cast<float>(n - i) * in1);
            tot0 += w[i] * izf * (rn1 * static_cast<float>(kShapInv.v[n - i]));
          }
        }
        total = one ? tot1 : tot0;
      } else {
        total = MT(0);
        if (one) {
          MT next = wn;
#pragma unroll
          for (int i = MAXN - 1; i >= 0; --i) {
            if (i < n) {
              const MT tmp = next * (rn1 * static_cast<MT>(1.0 / (double)(i + 1)));
              total += tmp;
              next = w[i] - tmp * zf * (static_cast<MT>(n - i) * in1);
            }
          }
        } else {
          const MT izf = MT(1) / zf;
#pragma unroll
          for (int i = MAXN - 1; i >= 0; --i) {
            if (i < n) total += w[i] * izf * (rn1 * static_cast<MT>(kShapInv.v[n - i]));
          }
        }
      }
      out[(int64_t)om * kShapTabStride + e_i] = total * ((one ? MT(1) : MT(0)) - zf);
    }
  }
}

// Sum of the path slices' partials in slice order, / divisor, bias column.
template <typename ACC>
__global__ void __launch_bounds__(256) contrib_slices_kernel(
    const double* __restrict__ part, int32_t slices, int64_t rows, int32_t K, int32_t F,
    const double* __restrict__ bias, double divisor, ACC* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const int W = K * (F + 1);
  ACC* o = out + row * W;
  for (int g = 0; g < K; ++g) {
    for (int f = 0; f < F; ++f) {
      const int j = g * (F + 1) + f;
      double t = 0.0;
      for (int sl = 0; sl < slices; ++sl) t += part[((int64_t)sl * W + j) * rows + row];
      o[j] = (ACC)(t / divisor);
    }
    o[g * (F + 1) + F] = (ACC)bias[g];
  }
}

// SHAP interaction values (TI_OUTPUT_INTERACT), the off-diagonal part.  For a
// path with merged elements 0..n-1 (one fraction o_i = bit i of om, zero
// fraction z_i, leaf value v), conditioning on element j takes j out of the
// path and scales the leaf by o_j (on) or z_j (off), so for i != j
//   Phi[feat_j][feat_i] += 1/2 (o_j - z_j) (o_i - z_i) UnwoundPathSum_i(w^-j) v
// with w^-j the path weights of the n - 1 other elements (xgboost's TreeShap
// with condition = +-1, PredictInteractionContributions).
//
// One row per lane, path slices on blockIdx.y, as contrib_reg_kernel.
// blockIdx.z = g * nb + b names an output group g and a block of cpb =
// kShapLdsW / (F + 1) conditioned features [j0, j1); the block's accumulators
// [(j1 - j0) * (F + 1)][64] of MT are the LDS budget of contrib_reg_kernel.
// A path of another group (scalar leaves), of fewer than two elements or with
// no element in [j0, j1) is skipped under a scalar branch before any row is
// read.
//
// w^-j is extended from scratch over the elements other than j, not unwound
// from the full weights: the unwind divides by z_j where o_j = 0 and by o_j's
// chain where it is 1, which branches per lane and amplifies float32 error
// for small z_j; the extension is the arithmetic xgboost itself does under a
// condition, is uniform across the wave (j is a scalar), and costs
// n^2 / 2 multiply-adds beside the n^2 of the n - 1 unwound sums that follow
// either way.  The full weights w[0..n] are then never needed: the diagonal
// comes from the contributions (interact_finish_kernel).
//
// Raw partials go to part[slice][(g * F + feat_j) * (F + 1) + feat_i][rows];
// nothing is read back, no atomics.  The output type plays no part here, so
// the kernel is not instantiated per ACC.
template <typename XT, typename MT, int MAXN>
__global__ void __launch_bounds__(64) interact_reg_kernel(
    const XT* __restrict__ X, int64_t rows, int64_t stride, int32_t cols, int32_t zero_map_on,
    const ShapPath* __restrict__ paths, int64_t n_paths, const ShapElem* __restrict__ elems,
    const double* __restrict__ leafv, int32_t LW, int32_t K, int32_t F, int32_t cpb, int32_t nb,
    double* __restrict__ part, int64_t paths_per_slice, const ShapCatRef* __restrict__ cat_refs,
    const uint32_t* __restrict__ cat_words) {
  extern __shared__ double shap_lds[];
  const int lane = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * 64 + lane;
  const bool live = row < rows;
  const XT* xr = X + (live ? row : rows - 1) * stride;
  const int F1 = F + 1;
  const int g = (int)blockIdx.z / nb;
  const int j0 = ((int)blockIdx.z - g * nb) * cpb;
  const int j1 = j0 + cpb < F ? j0 + cpb : F;
  const int C = (j1 - j0) * F1;
  MT* acc = reinterpret_cast<MT*>(shap_lds) + lane;   // acc[c * 64]
  for (int c = 0; c < C; ++c) acc[c * 64] = MT(0);
  const int64_t p_begin = (int64_t)blockIdx.y * paths_per_slice;
  const int64_t p_end = p_begin + paths_per_slice < n_paths ? p_begin + paths_per_slice : n_paths;
  for (int64_t p = p_begin; p < p_end; ++p) {
    const ShapPath P = paths[p];
    const int n = P.n;
    if (n < 2 || (LW == 1 && P.group != g)) continue;
    const ShapElem* pe = elems + P.first;
    bool mine = false;
    for (int i = 0; i < n; ++i) {
      const int32_t fe = pe[i].feature;
      mine = mine || (fe >= j0 && fe < j1);
    }
    if (!mine) continue;
    uint32_t om = 0u;                             // one fractions, bit i = element i
    for (int i = 0; i < n; ++i) {
      const ShapElem e = pe[i];
      double x = e.feature < cols ? (double)xr[e.feature] : __builtin_nan("");
      if (zero_map_on && __builtin_fabs(x) <= (double)1e-35f) x = 0.0;
      om |= (shap_follow_num(e, x) ? 1u : 0u) << i;
    }
    if (cat_refs) {
      for (int i = 0; i < n; ++i) {
        const int32_t fe = pe[i].feature;
        const uint32_t fl = pe[i].flags;
        if (!(fl & kShapCat)) continue;
        const double x = fe < cols ? (double)xr[fe] : __builtin_nan("");
        if (!shap_follow_cat(fl, x, P.first + i, cat_refs, cat_words)) om &= ~(1u << i);
      }
    }
    const MT lv = static_cast<MT>(leafv[P.leaf * LW + (LW == 1 ? 0 : g)]);
    const int m = n - 1;                          // elements of the conditioned path
    const MT rm1 = static_cast<MT>(m + 1);
    const MT im1 = static_cast<MT>(kShapInv.v[m + 1]);
    for (int j = 0; j < n; ++j) {
      const int32_t fj = pe[j].feature;
      if (fj < j0 || fj >= j1) continue;
      // ExtendPath over the elements other than j
      MT w[MAXN];
      w[0] = MT(1);
#pragma unroll
      for (int d = 1; d < MAXN; ++d) {
        if (d <= m) {
          const int src = d - 1 + (d - 1 >= j ? 1 : 0);
          const MT of = ((om >> src) & 1u) ? MT(1) : MT(0);
          const MT zf = static_cast<MT>(pe[src].zf);
          w[d] = MT(0);
#pragma unroll
          for (int i = d - 1; i >= 0; --i) {
            w[i + 1] += of * w[i] * static_cast<MT>((double)(i + 1) / (double)(d + 1));
            w[i] = zf * w[i] * static_cast<MT>((double)(d - i) / (double)(d + 1));
          }
        }
      }
      MT wm = MT(0);                              // w[m]
#pragma unroll
      for (int i = 0; i < MAXN; ++i)
        if (i == m) wm = w[i];
      const MT oj = ((om >> j) & 1u) ? MT(1) : MT(0);
      const MT cj = MT(0.5) * (oj - static_cast<MT>(pe[j].zf)) * lv;
      MT* accj = acc + (fj - j0) * F1 * 64;
      for (int e_i = 0; e_i < n; ++e_i) {
        if (e_i == j) continue;
        // UnwoundPathSum of element e_i in w^-j: both branches, selected per
        // lane (the branch on `one` diverges within a wave anyway)
        const bool one = ((om >> e_i) & 1u) != 0u;
        const MT zf = static_cast<MT>(pe[e_i].zf);
        const MT izf = MT(1) / zf;
        MT next = wm, tot1 = MT(0), tot0 = MT(0);
#pragma unroll
        for (int i = MAXN - 2; i >= 0; --i) {
          if (i < m) {
            const MT tmp = next * (rm1 * static_cast<MT>(1.0 / (double)(i + 1)));
            tot1 += tmp;
            next = w[i] - tmp * zf * (static_cast<MT>(m - i) * im1);
            tot0 += w[i] * izf * (rm1 * static_cast<MT>(kShapInv.v[m - i]));
          }
        }
        const MT s = (one ? tot1 : tot0) * ((one ? MT(1) : MT(0)) - zf);
        accj[pe[e_i].feature * 64] += cj * s;
      }
    }
  }
  if (!live) return;
  const int64_t W2 = (int64_t)K * F * F1;
  double* pp = part + ((int64_t)blockIdx.y * W2 + (int64_t)(g * F + j0) * F1) * rows + row;
  for (int c = 0; c < C; ++c) pp[(int64_t)c * rows] = static_cast<double>(acc[c * 64]);
}

// One thread per (row, group, matrix row fj): the off-diagonal entries are
// the path slices' partials summed in slice order in float64 over the
// divisor; the diagonal is the feature's contribution (phi, launch_contrib's
// output) minus the off-diagonal entries as written, so a row of the matrix
// sums to the contribution; the bias row and column are zero but for
// Phi[F][F] = bias (xgboost's PredictInteractionContributions).
template <typename ACC>
__global__ void __launch_bounds__(64) interact_finish_kernel(
    const double* __restrict__ part, int32_t slices, int64_t rows, int32_t K, int32_t F,
    const ACC* __restrict__ phi, const double* __restrict__ bias, double divisor,
    ACC* __restrict__ out, int64_t out_ld) {
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= rows) return;
  const int F1 = F + 1;
  const int g = (int)blockIdx.y / F1;
  const int fj = (int)blockIdx.y - g * F1;
  ACC* o = out + row * out_ld + (int64_t)blockIdx.y * F1;   // out_ld: elements an output row
  if (fj == F) {
    for (int fi = 0; fi < F; ++fi) o[fi] = ACC(0);
    o[F] = (ACC)bias[g];
    return;
  }
  const int64_t W2 = (int64_t)K * F * F1;
  const int64_t c0 = (int64_t)(g * F + fj) * F1;
  double off = 0.0;
  for (int fi = 0; fi < F; ++fi) {
    if (fi == fj) continue;
    double t = 0.0;
    for (int sl = 0; sl < slices; ++sl) t += part[((int64_t)sl * W2 + c0 + fi) * rows + row];
    const ACC v = (ACC)(t / divisor);
    o[fi] = v;
    off += static_cast<double>(v);
  }
  o[fj] = (ACC)(static_cast<double>(phi[row * K * F1 + blockIdx.y]) - off);
  o[F] = ACC(0);
}

namespace {

int ensure_lds_attr(int device, KernelFn fn);   // treeinfer.hip
void occ_note(KernelFn fn, int block, size_t lds);

// the TreeSHAP buffers of one replica (device current), after a failed upload
// or with the replica; the caller restores `bytes`
void free_shap(DeviceForest& d) {
  d.shap_mem.release();
  static_cast<ShapPtrs&>(d) = ShapPtrs();
  d.shap_tab_state = 0;
}

// TreeSHAP path tables + bias (see ShapPath).  Forests without covers or
// with XGBoost-rule categorical splits get none (TI_OUTPUT_CONTRIB is then
// unsupported).
//
// The categorical part of an element is a set of codes `allow` (words, bit
// v % 32 of word v / 32) plus kShapCatOutside, which says what happens to
// every value the words do not cover.  Before the first categorical split
// the element allows everything: no words, outside set.  With S the node's
// bitset (LightGBM's rule: in S -> left; NaN, x <= -1, x >= 2^31 and codes
// past S's last word -> right):
//   right turn: allow \= S.  Nothing outside S's words is lost, so the words
//               grow to max(own, S's) while outside is set, and stay otherwise.
//   left turn:  allow &= S.  Nothing past S's words follows: the words are cut
//               to S's length (words the set did not have yet are S's own
//               where outside was set, nothing otherwise) and outside clears.
// A set may end up empty with outside clear: an element no row follows.
struct ShapBuilder {
  struct Elem {
    ShapElem e;
    std::vector<uint32_t> allow;   // kShapCat elements only
  };
  const ti_forest_desc* d;
  ti_forest* f;
  int64_t b = 0;
  int group = 0;
  std::vector<Elem> cur;

  static void cat_turn(Elem& el, const uint32_t* s, size_t ns, bool left) {
    const bool outside = !(el.e.flags & kShapCat) || (el.e.flags & kShapCatOutside);
    const uint32_t fill = outside ? ~0u : 0u;
    std::vector<uint32_t>& a = el.allow;
    const size_t len = a.size();
    if (left) {
      a.resize(outside ? ns : std::min(len, ns), fill);
      for (size_t w = 0; w < a.size(); ++w) a[w] &= s[w];
      el.e.flags &= ~kShapCatOutside;
    } else {
      if (outside) a.resize(std::max(len, ns), fill);
      for (size_t w = 0; w < std::min(a.size(), ns); ++w) a[w] &= ~s[w];
      if (outside) el.e.flags |= kShapCatOutside;
    }
    el.e.flags |= kShapCat;
  }

  void dfs(int32_t v) {
    const int64_t g = b + v;
    const int LW = d->leaf_width;
    if (d->feature[g] < 0) {
      ShapPath p;
      p.group = group;
      p.n = static_cast<int32_t>(cur.size());
      p.first = static_cast<int64_t>(f->h_elems.size());
      p.leaf = static_cast<int64_t>(f->h_path_leaf.size()) / LW;
      for (const Elem& el : cur) {
        f->h_elems.push_back(el.e);
        if (!f->has_cat) continue;   // no categorical node in the forest: no refs at all
        f->h_shap_cat_refs.push_back(ShapCatRef{static_cast<uint32_t>(f->h_shap_cat.size()),
                                                static_cast<uint32_t>(el.allow.size())});
        f->h_shap_cat.insert(f->h_shap_cat.end(), el.allow.begin(), el.allow.end());
      }
      for (int k = 0; k < LW; ++k) f->h_path_leaf.push_back(d->leaf_value[g * LW + k]);
      f->h_paths.push_back(p);
      f->shap_maxl = std::max(f->shap_maxl, p.n);
      return;
    }
    const int32_t fe = d->feature[g];
    const double t = d->threshold[g];
    const bool cat = (d->flags[g] & TI_NODE_CATEGORICAL) != 0;
    const bool nan_left = (d->flags[g] & TI_NODE_NAN_LEFT) != 0;
    const bool zero_left = (d->flags[g] & TI_NODE_ZERO_FLIP) ? !(0 <= t) : (0 <= t);
    for (int side = 0; side < 2; ++side) {
      const bool left = side == 0;
      const int32_t child = left ? d->left[g] : d->right[g];
      const std::vector<Elem> saved = cur;
      Elem el{ShapElem{fe, kShapNanOk | kShapZeroOk, std::nan(""), INFINITY, 1.0}, {}};
      for (size_t i = 0; i < cur.size(); ++i)
        if (cur[i].e.feature == fe) {   // unwind the earlier split on fe (interval and set),
          el = cur[i];                  // re-extend at the end
          cur.erase(cur.begin() + static_cast<std::ptrdiff_t>(i));
          break;
        }
      ShapElem& e = el.e;
      e.zf = (d->cover[b + child] / d->cover[g]) * e.zf;
      if (cat) {
        // the interval and the NaN / zero flags belong to the numerical splits
        cat_turn(el, d->cat_bits + d->cat_offset[g], static_cast<size_t>(d->cat_nwords[g]), left);
      } else {
        if (left) {
          if (std::isnan(t)) e.flags |= kShapEmpty;
          else e.hi = std::min(e.hi, t);
        } else if (!std::isnan(t)) {
          e.lo = std::isnan(e.lo) ? t : std::max(e.lo, t);   // -inf itself is a bound: x > -inf
        }
        if (nan_left != left) e.flags &= ~kShapNanOk;
        if (zero_left != left) e.flags &= ~kShapZeroOk;
      }
      cur.push_back(std::move(el));
      dfs(child);
      cur = saved;
    }
  }

  std::vector<double> mean(int32_t v) {   // FillNodeMeanValues, per leaf-vector entry
    const int64_t g = b + v;
    const int LW = d->leaf_width;
    std::vector<double> r(LW);
    if (d->feature[g] < 0) {
      for (int k = 0; k < LW; ++k) r[k] = d->leaf_value[g * LW + k];
      return r;
    }
    const int32_t l = d->left[g], rr = d->right[g];
    const std::vector<double> ml = mean(l), mr = mean(rr);
    for (int k = 0; k < LW; ++k)
      r[k] = (ml[k] * d->cover[b + l] + mr[k] * d->cover[b + rr]) / d->cover[g];
    return r;
  }
};

// At create: whether contributions are possible (covers; categorical nodes
// all with LightGBM's rule), and the host copy build_shap will read on first
// use.  The element's category set is LightGBM's membership test; a forest
// with an XGBoost-rule node (TI_NODE_CAT_XGB: in the set -> right, invalid
// codes left, NaN by flag) is refused.
void keep_shap_source(const ti_forest_desc* d, ti_forest* f) {
  f->shap_refused = 1;
  if (!d->cover) return;
  f->shap_refused = 2;
  if (f->has_cat_xgb) return;
  f->shap_refused = 0;
  auto src = std::make_unique<ti_forest::ShapSource>();
  const int64_t N = d->n_nodes, T = d->n_trees;
  src->tree_offset.assign(d->tree_offset, d->tree_offset + T + 1);
  if (d->tree_group) src->tree_group.assign(d->tree_group, d->tree_group + T);
  src->feature.assign(d->feature, d->feature + N);
  src->left.assign(d->left, d->left + N);
  src->right.assign(d->right, d->right + N);
  src->threshold.assign(d->threshold, d->threshold + N);
  src->leaf_value.assign(d->leaf_value, d->leaf_value + N * d->leaf_width);
  src->base_margin.assign(d->base_margin, d->base_margin + d->n_groups);
  src->cover.assign(d->cover, d->cover + N);
  src->flags.assign(d->flags, d->flags + N);
  src->desc = *d;
  src->desc.tree_offset = src->tree_offset.data();
  src->desc.tree_group = src->tree_group.empty() ? nullptr : src->tree_group.data();
  src->desc.feature = src->feature.data();
  src->desc.left = src->left.data();
  src->desc.right = src->right.data();
  src->desc.threshold = src->threshold.data();
  src->desc.leaf_value = src->leaf_value.data();
  src->desc.base_margin = src->base_margin.data();
  src->desc.cover = src->cover.data();
  src->desc.flags = src->flags.data();
  src->desc.leaf_id = nullptr;
  src->desc.cat_bits = nullptr;
  src->desc.cat_offset = nullptr;
  src->desc.cat_nwords = nullptr;
  if (f->has_cat) {   // the bitsets whole: a tree subset's offsets still point into them
    src->cat_bits.assign(d->cat_bits, d->cat_bits + d->n_cat_words);
    src->cat_offset.assign(d->cat_offset, d->cat_offset + N);
    src->cat_nwords.assign(d->cat_nwords, d->cat_nwords + N);
    src->desc.cat_bits = src->cat_bits.data();
    src->desc.cat_offset = src->cat_offset.data();
    src->desc.cat_nwords = src->cat_nwords.data();
  }
  f->shap_src = std::move(src);
  f->has_shap = 1;
}

void build_shap(const ti_forest_desc* d, ti_forest* f) {
  const int K = d->n_groups;
  std::vector<double> bias(K);
  for (int k = 0; k < K; ++k) bias[k] = d->base_margin[k] * d->average_divisor;
  ShapBuilder sb{d, f};
  for (int t = 0; t < d->n_trees; ++t) {
    sb.b = d->tree_offset[t];
    sb.group = d->leaf_width == 1 ? d->tree_group[t] : 0;
    sb.cur.clear();
    sb.dfs(0);
    const std::vector<double> m = sb.mean(0);
    if (d->leaf_width == 1) bias[sb.group] += m[0];
    else for (int k = 0; k < K; ++k) bias[k] += m[k];
  }
  f->h_shap_bias.resize(K);
  for (int k = 0; k < K; ++k) f->h_shap_bias[k] = bias[k] / d->average_divisor;
  f->shap_npaths = static_cast<int64_t>(f->h_paths.size());
}

// TI_OUTPUT_CONTRIB on one (unchunked) forest.  contrib_reg_kernel when the
// row's accumulators fit LDS (K * (F + 1) <= kShapLdsW) and paths have <= 32
// unique features: path slices over blockIdx.y, partials summed in slice
// order by contrib_slices_kernel.  Otherwise contrib_kernel, whose float32
// forests accumulate in a float64 scratch.
// First contributions call: build the path tables on the host and upload them
// to every device replica (under the forest's lock; later calls see
// shap_ready and skip it).
int ensure_shap(ti_forest* f) {
  if (f->shap_ready.load(std::memory_order_acquire)) return TI_OK;
  std::lock_guard<std::mutex> lk(f->shap_mu);
  if (f->shap_ready.load(std::memory_order_relaxed)) return TI_OK;
  if (f->h_paths.empty()) build_shap(&f->shap_src->desc, f);
  if (f->h_shap_cat.size() > std::numeric_limits<uint32_t>::max())
    return fail(TI_ERR_UNSUPPORTED, "the category sets of the TreeSHAP paths exceed 2^32 words");
  // the coefficient table's shape (contrib_reg_kernel TAB): paths of <= 8
  // unique features, 2^n x 8 coefficients each (padded), in the path
  // arithmetic's type.  The table itself is built per replica, later, by
  // ensure_shap_table.
  {
    const int mt = (f->accum != TI_F64 && !env_int("TI_SHAP_F64", 0)) ? 4 : 8;
    const int64_t W = static_cast<int64_t>(f->K) * (f->F + 1);
    f->h_tab_off.assign(f->h_paths.size(), 0);
    int64_t len = 0;
    bool ok = W <= kShapLdsW && f->shap_maxl <= kShapTabStride && !f->h_paths.empty();
    for (size_t i = 0; ok && i < f->h_paths.size(); ++i) {
      f->h_tab_off[i] = len;
      len += (int64_t(1) << f->h_paths[i].n) * kShapTabStride;
    }
    f->shap_tab_mt = ok ? mt : 0;
    f->shap_tab_len = ok ? len : 0;
    if (!ok) f->h_tab_off.clear();
  }
  int dev0 = 0;
  TI_HIP(hipGetDevice(&dev0));
  int rc = TI_OK;
  // each replica's byte count before the uploads: a failure restores it, so
  // ti_forest_info's device_bytes does not keep the freed tables
  std::vector<int64_t> bytes0;
  for (auto& dp : f->devs) bytes0.push_back(dp->bytes);
  for (auto& dp : f->devs) {
    DeviceForest& d = *dp;
    if ((rc = fail_hip(hipSetDevice(d.device), "hipSetDevice"))) break;
    if ((rc = upload(&d.shap_mem, &d.shap_paths, f->h_paths, &d.bytes)) ||
        (rc = upload(&d.shap_mem, &d.shap_elems, f->h_elems, &d.bytes)) ||
        (rc = upload(&d.shap_mem, &d.shap_leaf, f->h_path_leaf, &d.bytes)) ||
        (rc = upload(&d.shap_mem, &d.shap_bias, f->h_shap_bias, &d.bytes)) ||
        (rc = upload(&d.shap_mem, &d.shap_cat_refs, f->h_shap_cat_refs, &d.bytes)) ||
        (rc = upload(&d.shap_mem, &d.shap_cat_words, f->h_shap_cat, &d.bytes)))
      break;
  }
  if (rc) {
    // nothing half-built survives: every replica's path tables are freed (the
    // host tables stay, so the next call retries from them)
    const std::string err = g_last_error;
    for (size_t i = 0; i < f->devs.size(); ++i) {
      (void)hipSetDevice(f->devs[i]->device);
      free_shap(*f->devs[i]);
      f->devs[i]->bytes = bytes0[i];
    }
    (void)hipGetLastError();
    (void)hipSetDevice(dev0);
    return fail(rc, err);
  }
  TI_HIP(hipSetDevice(dev0));
  f->h_paths.clear(); f->h_paths.shrink_to_fit();
  f->h_elems.clear(); f->h_elems.shrink_to_fit();
  f->h_path_leaf.clear(); f->h_path_leaf.shrink_to_fit();
  f->h_shap_cat_refs.clear(); f->h_shap_cat_refs.shrink_to_fit();
  f->h_shap_cat.clear(); f->h_shap_cat.shrink_to_fit();
  f->shap_src.reset();
  f->shap_ready.store(true, std::memory_order_release);
  return TI_OK;
}

// The coefficient table of one replica (device d.device current), built on
// the first contributions batch that would use it.  It is an optimisation
// only: any failure (over the size cap, allocation, launch) frees what was
// allocated, clears the HIP error and marks the replica, whose contributions
// then take the extend / unwind kernel -- never an error for the caller.  The
// build runs on a private stream and waits for that stream alone.
void ensure_shap_table(ti_forest* f, DeviceForest& d) {
  std::lock_guard<std::mutex> lk(f->shap_mu);
  if (d.shap_tab_state != 0) return;
  d.shap_tab_state = -1;
  const size_t bytes = static_cast<size_t>(f->shap_tab_len) * f->shap_tab_mt;
  if (!f->shap_tab_mt || f->shap_tab_mb <= 0 ||
      bytes > (static_cast<size_t>(f->shap_tab_mb) << 20))
    return;
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t s = nullptr;
  bool ok = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
  int64_t up = 0;
  DeviceAllocs mem;   // the table's two buffers: joined to shap_mem once built
  ok = ok && !env_int("TI_SHAP_TABLE_FAULT", 0) &&   // fault injection (tests)
       upload(&mem, &d.shap_tab_off, f->h_tab_off, &up) == TI_OK &&
       hipMalloc(&d.shap_tab, std::max<size_t>(bytes, 16)) == hipSuccess;
  if (ok) mem.ptrs.push_back(d.shap_tab);
  if (ok) {
    const unsigned np = static_cast<unsigned>(f->h_tab_off.size());
    if (f->shap_tab_mt == 4)
      hipLaunchKernelGGL((shap_table_kernel<float, 16>), dim3(np), dim3(256), 0, s,
                         d.shap_paths, d.shap_elems, d.shap_tab_off, static_cast<float*>(d.shap_tab));
    else
      hipLaunchKernelGGL((shap_table_kernel<double, 16>), dim3(np), dim3(256), 0, s,
                         d.shap_paths, d.shap_elems, d.shap_tab_off, static_cast<double*>(d.shap_tab));
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  }
  if (s) (void)hipStreamDestroy(s);
  if (!ok) {
    mem.release();
    d.shap_tab = nullptr;
    d.shap_tab_off = nullptr;
    (void)hipGetLastError();
    return;
  }
  d.shap_mem.ptrs.insert(d.shap_mem.ptrs.end(), mem.ptrs.begin(), mem.ptrs.end());
  d.bytes += up + static_cast<int64_t>(bytes);
  d.shap_tab_state = 1;
  f->shap_tab_build_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// use_table = false keeps a call on the extend / unwind arithmetic whatever
// the batch size (launch_interact: see there).
int launch_contrib(ti_forest* f, DeviceForest& d, const void* X, int xdt, int64_t rows,
                   int32_t cols, int64_t stride, void* out, hipStream_t stream,
                   bool use_table = true) {
  if (!f->has_shap)
    return fail(TI_ERR_UNSUPPORTED,
                f->shap_refused == 2
                    ? "contributions of categorical splits with XGBoost's rule (TI_NODE_CAT_XGB) are "
                      "not supported; categorical splits with LightGBM's rule are"
                    : "contributions need node covers (ti_forest_desc.cover)");
  {
    const int rc = ensure_shap(f);
    if (rc) return rc;
  }
  const int64_t W = static_cast<int64_t>(f->K) * (f->F + 1);
  const int64_t n_paths = static_cast<int64_t>(d.shap_paths ? 1 : 0) * f->shap_npaths;
  const int force_generic = env_int("TI_SHAP_GENERIC", 0);
  if (W <= kShapLdsW && f->shap_maxl <= 32 && !force_generic) {
    // registers + LDS accumulators: no scratch accumulator, no memset
    const int maxn = f->shap_maxl <= 8 ? 8 : f->shap_maxl <= 16 ? 16 : 32;
    const int force_f64 = env_int("TI_SHAP_F64", 0);
    const bool f32_math = f->accum != TI_F64 && !force_f64 && maxn <= kShapF32MaxN;
    const size_t lds_w = static_cast<size_t>(W) * 64 * (f32_math ? 4 : 8);
    const unsigned grid_r = static_cast<unsigned>((rows + 63) / 64);
    if (rows == 0) return TI_OK;
    // Path slices: one 64-row wave walks n_paths / slices paths, so a small
    // batch still fills the 256 CUs (>= kShapWaveTarget waves); partials
    // [slices][W][rows] are summed in slice order by contrib_slices_kernel.
    const int force_slices = env_int("TI_SHAP_SLICES", 0);
    int64_t slices = force_slices > 0 ? force_slices
                                      : (kShapWaveTarget + grid_r - 1) / static_cast<int64_t>(grid_r);
    slices = std::min<int64_t>(slices, std::max<int64_t>(1, n_paths / kShapMinPathsPerSlice));
    slices = std::min<int64_t>(slices, kShapMaxSlices);
    while (slices > 1 && static_cast<uint64_t>(slices) * W * rows * 8 > kShapPartBytesMax) --slices;
    slices = std::max<int64_t>(slices, 1);
    const int64_t pps = (n_paths + slices - 1) / slices;
    // the coefficient table pays off for small batches (C2 model: 4,096 rows
    // 4.1e5 vs 2.7e5 rows/s); at 100k rows its gathers (a 64-row wave reads
    // most of each path's 2^n x 32 B block) make it slower than the extend /
    // unwind arithmetic (2.2e5 vs 2.9e5): profiles/r3_shap_table.jsonl
    const bool want_tab = use_table && f->shap_tab_mt != 0 && rows <= f->shap_tab_rows;
    if (want_tab && d.shap_tab_state == 0) ensure_shap_table(f, d);
    ScratchHold part_buf(d, stream);   // given back behind contrib_slices_kernel
    if (slices > 1 && !part_buf.take(static_cast<size_t>(slices * W * rows) * 8))
      return fail(TI_ERR_NOMEM, "slice partials allocation failed");
    double* part = static_cast<double*>(part_buf.p);
#define TI_CONTRIB_REG(XT_, ACC_, MT_, N_)                                                          \
  do {                                                                                         \
    const bool tab_ = want_tab && d.shap_tab_state == 1 &&                                     \
                      f->shap_tab_mt == (int)sizeof(MT_);                                      \
    KernelFn fn_ = tab_ ? reinterpret_cast<KernelFn>(contrib_reg_kernel<XT_, ACC_, MT_, 8, true>) \
                        : reinterpret_cast<KernelFn>(contrib_reg_kernel<XT_, ACC_, MT_, N_>);  \
    int rc_ = ensure_lds_attr(d.device, fn_);                                                  \
    if (rc_) return rc_;                                                                       \
    if (tab_)                                                                                  \
      hipLaunchKernelGGL((contrib_reg_kernel<XT_, ACC_, MT_, 8, true>), dim3(grid_r, (unsigned)slices), \
                         dim3(64), lds_w, stream,                                              \
                         static_cast<const XT_*>(X), rows, stride, cols, f->lgb_zero_map,      \
                         d.shap_paths, n_paths, d.shap_elems, d.shap_leaf, f->LW, f->K, f->F,  \
                         f->shap_maxl, d.shap_bias, f->divisor, part, pps, static_cast<ACC_*>(out), \
                         static_cast<const MT_*>(d.shap_tab), d.shap_tab_off,                  \
                         d.shap_cat_refs, d.shap_cat_words);                                   \
    else                                                                                       \
      hipLaunchKernelGGL((contrib_reg_kernel<XT_, ACC_, MT_, N_>), dim3(grid_r, (unsigned)slices), dim3(64), \
                         lds_w, stream,                                                        \
                         static_cast<const XT_*>(X), rows, stride, cols, f->lgb_zero_map,      \
                         d.shap_paths, n_paths, d.shap_elems, d.shap_leaf, f->LW, f->K, f->F,  \
                         f->shap_maxl, d.shap_bias, f->divisor, part, pps, static_cast<ACC_*>(out), \
                         static_cast<const MT_*>(nullptr), static_cast<const int64_t*>(nullptr), \
                         d.shap_cat_refs, d.shap_cat_words);                                   \
    if (part) {                                                                                \
      const unsigned g2 = static_cast<unsigned>((rows + 255) / 256);                           \
      hipLaunchKernelGGL((contrib_slices_kernel<ACC_>), dim3(g2), dim3(256), 0, stream, part,  \
                         (int32_t)slices, rows, f->K, f->F, d.shap_bias, f->divisor,           \
                         static_cast<ACC_*>(out));                                             \
    }                                                                                          \
  } while (0)
#define TI_CONTRIB_REG_N(XT_, ACC_, MT_)                     \
  do {                                                       \
    if (maxn == 8) TI_CONTRIB_REG(XT_, ACC_, MT_, 8);        \
    else if (maxn == 16) TI_CONTRIB_REG(XT_, ACC_, MT_, 16); \
    else TI_CONTRIB_REG(XT_, ACC_, MT_, 32);                 \
  } while (0)
#define TI_CONTRIB_REG_F32(XT_)                              \
  do {                                                       \
    if (maxn == 8) TI_CONTRIB_REG(XT_, float, float, 8);     \
    else TI_CONTRIB_REG(XT_, float, float, 16);              \
  } while (0)
    // Path arithmetic in the forest's accumulator type: float64 for LightGBM
    // and sklearn; float32 for XGBoost, whose TreeShap keeps its path
    // elements and contributions in bst_float, on paths of at most
    // kShapF32MaxN elements (longer ones, and TI_SHAP_F64=1, take float64).
    // Each slice accumulates in that type in LDS (float32 halves the LDS per
    // workgroup: 2x workgroups per CU); slices sum in float64.
    if (xdt == TI_F32) {
      if (f->accum == TI_F64) TI_CONTRIB_REG_N(float, double, double);
      else if (f32_math) TI_CONTRIB_REG_F32(float);
      else TI_CONTRIB_REG_N(float, float, double);
    } else {
      if (f->accum == TI_F64) TI_CONTRIB_REG_N(double, double, double);
      else if (f32_math) TI_CONTRIB_REG_F32(double);
      else TI_CONTRIB_REG_N(double, float, double);
    }
#undef TI_CONTRIB_REG_F32
#undef TI_CONTRIB_REG_N
#undef TI_CONTRIB_REG
    TI_HIP(hipGetLastError());
    return TI_OK;
  }
  double* acc = nullptr;
  ScratchHold acc_buf(d, stream);   // given back behind contrib_kernel
  if (f->accum == TI_F64) {
    acc = static_cast<double*>(out);
  } else {
    if (!acc_buf.take(static_cast<size_t>(rows * W) * 8))
      return fail(TI_ERR_NOMEM, "contributions accumulator allocation failed");
    acc = static_cast<double*>(acc_buf.p);
  }
  TI_HIP(hipMemsetAsync(acc, 0, static_cast<size_t>(rows * W) * 8, stream));
  const size_t lds = static_cast<size_t>(2 * f->shap_maxl + 1) * 64 * 8;
  KernelFn fn;
  if (xdt == TI_F32)
    fn = f->accum == TI_F64 ? reinterpret_cast<KernelFn>(contrib_kernel<float, double>)
                            : reinterpret_cast<KernelFn>(contrib_kernel<float, float>);
  else
    fn = f->accum == TI_F64 ? reinterpret_cast<KernelFn>(contrib_kernel<double, double>)
                            : reinterpret_cast<KernelFn>(contrib_kernel<double, float>);
  int rc = ensure_lds_attr(d.device, fn);
  if (rc) return rc;
  const unsigned grid = static_cast<unsigned>((rows + 63) / 64);
  if (xdt == TI_F32) {
    if (f->accum == TI_F64)
      hipLaunchKernelGGL((contrib_kernel<float, double>), dim3(grid), dim3(64), lds, stream,
                         static_cast<const float*>(X), rows, stride, cols, f->lgb_zero_map,
                         d.shap_paths, n_paths, d.shap_elems, d.shap_leaf, f->LW, f->K, f->F,
                         f->shap_maxl, d.shap_bias, f->divisor, acc, static_cast<double*>(out),
                         d.shap_cat_refs, d.shap_cat_words);
    else
      hipLaunchKernelGGL((contrib_kernel<float, float>), dim3(grid), dim3(64), lds, stream,
                         static_cast<const float*>(X), rows, stride, cols, f->lgb_zero_map,
                         d.shap_paths, n_paths, d.shap_elems, d.shap_leaf, f->LW, f->K, f->F,
                         f->shap_maxl, d.shap_bias, f->divisor, acc, static_cast<float*>(out),
                         d.shap_cat_refs, d.shap_cat_words);
  } else {
    if (f->accum == TI_F64)
      hipLaunchKernelGGL((contrib_kernel<double, double>), dim3(grid), dim3(64), lds, stream,
                         static_cast<const double*>(X), rows, stride, cols, f->lgb_zero_map,
                         d.shap_paths, n_paths, d.shap_elems, d.shap_leaf, f->LW, f->K, f->F,
                         f->shap_maxl, d.shap_bias, f->divisor, acc, static_cast<double*>(out),
                         d.shap_cat_refs, d.shap_cat_words);
    else
      hipLaunchKernelGGL((contrib_kernel<double, float>), dim3(grid), dim3(64), lds, stream,
                         static_cast<const double*>(X), rows, stride, cols, f->lgb_zero_map,
                         d.shap_paths, n_paths, d.shap_elems, d.shap_leaf, f->LW, f->K, f->F,
                         f->shap_maxl, d.shap_bias, f->divisor, acc, static_cast<float*>(out),
                         d.shap_cat_refs, d.shap_cat_words);
  }
  TI_HIP(hipGetLastError());
  return TI_OK;
}

// TI_OUTPUT_INTERACT on one (unchunked) forest: [rows, K, F + 1, F + 1].  The
// contributions go to a scratch through launch_contrib; interact_reg_kernel
// writes the off-diagonal partials of one row block and
// interact_finish_kernel assembles the block's matrices.  A row block is as
// many 64-row waves as keep one slice of partials within kShapPartBytesMax
// (path slices are dropped first, as for contributions).  There is no generic
// kernel: a matrix row wider than kShapLdsW, or a path of more than 32
// features, is refused.  out_ld is the output's row pitch in elements: K * (F
// + 1)^2, or the whole forest's row when f is a group part that writes its
// groups' matrices in place (launch_chunked).
int launch_interact(ti_forest* f, DeviceForest& d, const void* X, int xdt, int64_t rows,
                    int32_t cols, int64_t stride, void* out, int64_t out_ld, hipStream_t stream) {
  if (!f->has_shap)
    return fail(TI_ERR_UNSUPPORTED,
                f->shap_refused == 2
                    ? "interactions of categorical splits with XGBoost's rule (TI_NODE_CAT_XGB) are "
                      "not supported; categorical splits with LightGBM's rule are"
                    : "interactions need node covers (ti_forest_desc.cover)");
  {
    const int rc = ensure_shap(f);
    if (rc) return rc;
  }
  const int F = f->F, F1 = F + 1, K = f->K;
  if (F1 > kShapLdsW)
    return fail(TI_ERR_UNSUPPORTED, "interactions need n_features + 1 <= " + std::to_string(kShapLdsW) +
                                        " (one matrix row of accumulators in LDS); the forest has " +
                                        std::to_string(F) + " features");
  if (f->shap_maxl > 32)
    return fail(TI_ERR_UNSUPPORTED, "interactions need paths of at most 32 unique features; the "
                                    "forest's longest has " + std::to_string(f->shap_maxl));
  if (rows == 0) return TI_OK;
  const size_t as = f->accum == TI_F64 ? 8 : 4;
  const size_t xs = xdt == TI_F64 ? 8 : 4;
  const int64_t n_paths = static_cast<int64_t>(d.shap_paths ? 1 : 0) * f->shap_npaths;
  const int maxn = f->shap_maxl <= 8 ? 8 : f->shap_maxl <= 16 ? 16 : 32;
  const bool f32_math = f->accum != TI_F64 && !env_int("TI_SHAP_F64", 0) && maxn <= kShapF32MaxN;
  const int cpb = kShapLdsW / F1;                    // conditioned features a block
  const int nb = F > 0 ? (F + cpb - 1) / cpb : 0;    // blocks a group
  const size_t lds = static_cast<size_t>(std::min(cpb, std::max(F, 1)) * F1) * 64 * (f32_math ? 4 : 8);
  const int64_t W2 = static_cast<int64_t>(K) * F * F1;   // partial columns
  // TI_SHAP_PART_MB (developer knob): the partials' bound, so that a test
  // reaches the row-block loop without a 2 GiB batch
  const int part_mb = env_int("TI_SHAP_PART_MB", 0);
  const uint64_t part_max = part_mb > 0 ? static_cast<uint64_t>(part_mb) << 20 : kShapPartBytesMax;
  int64_t rb = static_cast<int64_t>(part_max / static_cast<uint64_t>(std::max<int64_t>(W2, 1) * 8));
  rb = std::min(rows, std::max<int64_t>(64, rb / 64 * 64));
  const int64_t grid_rb = (rb + 63) / 64;
  const int64_t waves = grid_rb * std::max(K * nb, 1);
  const int force_slices = env_int("TI_SHAP_SLICES", 0);
  // TI_SHAP_SLICES (developer knob) names the count outright, for forests of
  // any size; otherwise enough slices to fill the device, of at least
  // kShapMinPathsPerSlice paths each
  int64_t slices = force_slices > 0
                       ? std::min<int64_t>(force_slices, std::max<int64_t>(n_paths, 1))
                       : std::min<int64_t>((kShapWaveTarget + waves - 1) / waves,
                                           std::max<int64_t>(1, n_paths / kShapMinPathsPerSlice));
  slices = std::min<int64_t>(slices, kShapMaxSlices);
  while (slices > 1 && static_cast<uint64_t>(slices) * W2 * rb * 8 > part_max) --slices;
  slices = std::max<int64_t>(slices, 1);
  const int64_t pps = (n_paths + slices - 1) / slices;
  // The call's scratch: the contributions [rows, K * (F + 1)] of the output
  // type, then the partials of one row block, in the replica's own grow-only
  // buffer.  Every kernel that writes or reads it is launched below on
  // `stream`, in order; a later call, on any stream, first waits for
  // interact_done, which this call records behind its last kernel, and the
  // buffer grows only after that event has completed.  interact_mu covers
  // the hand-over (wait, grow, launches, record), not the kernels' run.
  const size_t phi_bytes = (static_cast<size_t>(rows) * K * F1 * as + 255) & ~size_t(255);
  const size_t part_bytes = static_cast<size_t>(slices * W2 * rb) * 8;
  std::lock_guard<std::mutex> scratch_lk(d.interact_mu);
  if (!d.interact_done) {
    TI_HIP(hipEventCreateWithFlags(&d.interact_done, hipEventDisableTiming));
  } else if (phi_bytes + part_bytes > d.interact_cap) {
    TI_HIP(hipEventSynchronize(d.interact_done));
  } else {
    TI_HIP(hipStreamWaitEvent(stream, d.interact_done, 0));
  }
  if (phi_bytes + part_bytes > d.interact_cap) {
    if (d.interact_buf) (void)hipFree(d.interact_buf);
    d.interact_buf = nullptr;
    d.interact_cap = 0;
    const size_t want_cap = std::max<size_t>(phi_bytes + part_bytes, size_t(1) << 20);
    if (hipMalloc(&d.interact_buf, want_cap) != hipSuccess) {
      (void)hipGetLastError();
      return fail(TI_ERR_NOMEM, "interaction scratch allocation failed");
    }
    d.interact_cap = want_cap;
  }
  unsigned char* scratch = static_cast<unsigned char*>(d.interact_buf);
  void* phi = scratch;
  double* part = reinterpret_cast<double*>(scratch + phi_bytes);
  // The contributions by arithmetic, never through the coefficient table: they
  // are a small share of this call (the interactions are about n times their
  // work), and a request for matrices then neither builds nor waits for a
  // table of up to TI_OPT_SHAP_TABLE_MB that contributions requests may never
  // ask for.
  int rc = launch_contrib(f, d, X, xdt, rows, cols, stride, phi, stream, false);
  if (rc) {
    (void)hipEventRecord(d.interact_done, stream);
    return rc;
  }
#define TI_INTERACT(XT_, MT_, N_)                                                                 \
  do {                                                                                            \
    KernelFn fn_ = reinterpret_cast<KernelFn>(interact_reg_kernel<XT_, MT_, N_>);                 \
    rc = ensure_lds_attr(d.device, fn_);                                                          \
    if (rc == TI_OK) {                                                                            \
      occ_note(fn_, 64, lds);                                                                     \
      hipLaunchKernelGGL((interact_reg_kernel<XT_, MT_, N_>),                                     \
                         dim3(grid_r, (unsigned)slices, (unsigned)(K * nb)), dim3(64), lds, stream, \
                         static_cast<const XT_*>(xb), n, stride, cols, f->lgb_zero_map,           \
                         d.shap_paths, n_paths, d.shap_elems, d.shap_leaf, f->LW, K, F, cpb, nb,  \
                         part, pps, d.shap_cat_refs, d.shap_cat_words);                           \
    }                                                                                             \
  } while (0)
#define TI_INTERACT_N(XT_, MT_)                       \
  do {                                                \
    if (maxn == 8) TI_INTERACT(XT_, MT_, 8);          \
    else if (maxn == 16) TI_INTERACT(XT_, MT_, 16);   \
    else TI_INTERACT(XT_, MT_, 32);                   \
  } while (0)
#define TI_INTERACT_F32(XT_)                          \
  do {                                                \
    if (maxn == 8) TI_INTERACT(XT_, float, 8);        \
    else TI_INTERACT(XT_, float, 16);                 \
  } while (0)
  for (int64_t r0 = 0; r0 < rows && rc == TI_OK; r0 += rb) {
    const int64_t n = std::min(rb, rows - r0);
    const unsigned grid_r = static_cast<unsigned>((n + 63) / 64);
    const void* xb = static_cast<const unsigned char*>(X) + static_cast<size_t>(r0 * stride) * xs;
    if (nb > 0) {
      // path arithmetic in the forest's accumulator type, float64 on paths of
      // more than kShapF32MaxN elements, as for contributions
      if (xdt == TI_F32) {
        if (f32_math) TI_INTERACT_F32(float);
        else TI_INTERACT_N(float, double);
      } else {
        if (f32_math) TI_INTERACT_F32(double);
        else TI_INTERACT_N(double, double);
      }
      if (rc) break;
    }
    const dim3 g2(grid_r, static_cast<unsigned>(K * F1));
    unsigned char* ob = static_cast<unsigned char*>(out) + static_cast<size_t>(r0 * out_ld) * as;
    const unsigned char* pb = static_cast<const unsigned char*>(phi) + static_cast<size_t>(r0) * K * F1 * as;
    if (f->accum == TI_F64)
      hipLaunchKernelGGL((interact_finish_kernel<double>), g2, dim3(64), 0, stream, part,
                         (int32_t)slices, n, K, F, reinterpret_cast<const double*>(pb), d.shap_bias,
                         f->divisor, reinterpret_cast<double*>(ob), out_ld);
    else
      hipLaunchKernelGGL((interact_finish_kernel<float>), g2, dim3(64), 0, stream, part,
                         (int32_t)slices, n, K, F, reinterpret_cast<const float*>(pb), d.shap_bias,
                         f->divisor, reinterpret_cast<float*>(ob), out_ld);
  }
#undef TI_INTERACT_F32
#undef TI_INTERACT_N
#undef TI_INTERACT
  if (rc == TI_OK && hipGetLastError() != hipSuccess)
    rc = fail(TI_ERR_DEVICE, "interaction kernel launch failed");
  (void)hipEventRecord(d.interact_done, stream);   // the next call's scratch waits for this one
  return rc;
}

}  // namespace
