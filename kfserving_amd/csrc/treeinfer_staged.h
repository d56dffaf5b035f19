// treeinfer_staged.h -- staged and iteration-range predictions in one pass,
// TI_OUTPUT_STAGED (ABI 14): the second of launch_staged's two
// stream-ordered passes (treeinfer.hip).
//
// A boosted forest is a sum of trees in a fixed order, one add a tree in the
// accumulator type: the answer after n trees is a snapshot of the chain the
// whole forest runs.  Pass 1 is the forest's own walk with TI_OUTPUT_LEAF into
// a [rows, T] int32 scratch.  Pass 2, here, reads no X: it replays the chain of
// trees [begin, ends[S-1]) once a row and writes it out at every stage end.
//
// Tables: leaf_base [T + 1] and a leaf table [sum over trees of (largest leaf
// id + 1)][LW] in the accumulator type, tree t's leaf of library id i at
// leaf_base[t] + i (treeinfer_approx.h's addressing), and the forest's resident
// tree_group [T].  The ends [S] come with each call.
//
// Work split.  The chain of a row is sequential, so the parallelism is rows: a
// lane a row, a wave 64 rows, a workgroup four waves that share nothing and
// never wait for each other -- every synchronisation is wave-local (a wavefront
// fence and s_wave_barrier, as tree_quantile_lds_kernel has it).
//
// Leaf ids.  The scratch is row-major: a lane reading its own row would touch
// 64 lines an instruction.  The wave reads the [64][kStTC] block of a chunk of
// kStTC trees coalesced along T (lane l, load i: element i * 64 + l) and puts
// it into its own LDS slice as [row][t] with a pitch of kStTC + 1 dwords, odd,
// so the lane-a-row reads that follow hit 64 distinct banks.  Two slices a
// wave: the global loads of chunk c + 1 are issued before the chain of chunk c
// runs and land in the other slice after it.
//
// The chain.  leaf_base[t], tree_group[t] and "is t + 1 a stage end" are the
// same for every lane: scalar loads and uniform branches.  Within a chunk the
// leaf-value gathers go out in batches (kGather trees: 8 scalar leaves, or 2
// vectors of up to 16 values), independent of the adds; the adds then run
// strictly in tree order through add_leaf<ACC, 16>, so the bits are the
// walk's.  (One output group: acc[0] + v alone, the add add_leaf<ACC, 1> and
// every select of add_leaf<ACC, 16> would make.)
//
// Stage ends.  finish_row -- base, divisor, transform -- runs on the
// accumulators as they stand, which it does not change, and writes its W
// results into the lane's row of an LDS output tile.  The tile's pitch is one
// element more than a row holds: an odd count of dwords for float, and for
// double an odd count of 8-byte words, which keeps every element 8-byte
// aligned (an odd dword pitch would not) and puts the 32 lanes of each half
// of a 64-bit LDS access on distinct bank pairs.  When the tile is full,
// and after the last stage, the wave stores it with consecutive lanes on
// consecutive elements of a row's contiguous S * W outputs.
//
// No atomics and no global read-modify-write: two calls give the same bits.
#pragma once

#include "treeinfer_kernels.h"

namespace ti {

constexpr int kStWaves = 4;              // waves a workgroup
constexpr int kStRows = kStWaves * 64;   // rows a workgroup
constexpr int kStTC = 16;                // trees per leaf-id chunk
constexpr int kStPitch = kStTC + 1;      // dwords per row of a slice
constexpr int kStKmax = kMaxGroups;

// Elements a row of the output tile holds: at least one stage, at least 64 bytes.
__host__ __device__ constexpr int staged_tile_elems(int width, size_t acc_bytes) {
  const int least = (int)(64 / acc_bytes);
  return width > least ? width : least;
}
// LDS of a workgroup: per wave two id slices and the output tile (pitch + 1 elements).
__host__ __device__ constexpr size_t staged_wave_lds(int tile_elems, size_t acc_bytes) {
  return 2 * 64 * kStPitch * 4 + (size_t)64 * (tile_elems + 1) * acc_bytes;
}

__device__ __forceinline__ void staged_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a.leaf_base / a.leaves: the tables above; a.st_*: the ids, the stages and
// the tile (KArgs).  blockDim.x = kStRows, kStWaves * staged_wave_lds bytes.
template <typename ACC, bool VEC>
__global__ void __launch_bounds__(kStRows, 2) staged_accum_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KMAX = kStKmax;
  constexpr int kGather = VEC ? 2 : 8;   // trees whose leaf values are in flight at once
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row0 = ((int64_t)blockIdx.x * kStWaves + wave) * 64;   // the wave's first row
  if (row0 >= a.n_rows) return;   // uniform over the wave; nobody waits for it
  const int64_t left_rows = a.n_rows - row0;
  const int rows_here = left_rows < 64 ? (int)left_rows : 64;

  const int OTE = a.st_tile;
  const int P = OTE + 1;   // tile pitch in elements
  unsigned char* mine = smem + (size_t)wave * staged_wave_lds(OTE, sizeof(ACC));
  int32_t* slice = reinterpret_cast<int32_t*>(mine);                       // [2][64][kStPitch]
  ACC* tile = reinterpret_cast<ACC*>(mine + 2 * 64 * kStPitch * 4);        // [64][P]

  const int T = a.n_trees;
  const int LW = a.leaf_width;
  const int K = a.n_groups;
  const int W = a.st_width;
  const int S = a.st_n;
  const int64_t SW = (int64_t)S * W;
  const int t_first = a.st_begin;
  const int t_last = a.st_ends[S - 1];   // the chain covers [t_first, t_last)
  const int slots = OTE / W;             // stages a tile holds
  const ACC* leaves = static_cast<const ACC*>(a.leaves);
  const int32_t* ids = a.st_leaf_ids + row0 * (int64_t)T;
  ACC* out = static_cast<ACC*>(a.out) + row0 * SW;

  // chunk c's block, coalesced: element e = i * 64 + lane is row e / kStTC,
  // tree t0 + e % kStTC.  A row past the batch or a tree past the chain reads
  // id 0, which every tree's table holds.
  auto load_chunk = [&](int t0, int32_t (&pre)[kStTC]) {
#pragma unroll
    for (int i = 0; i < kStTC; ++i) {
      const int e = i * 64 + lane;
      const int r = e / kStTC, j = e % kStTC;
      pre[i] = (r < rows_here && t0 + j < t_last) ? ids[(int64_t)r * T + t0 + j] : 0;
    }
  };
  auto store_chunk = [&](int32_t* sl, const int32_t (&pre)[kStTC]) {
#pragma unroll
    for (int i = 0; i < kStTC; ++i) {
      const int e = i * 64 + lane;
      sl[(e / kStTC) * kStPitch + e % kStTC] = pre[i];
    }
  };
  // the tile's `used` stages go out: consecutive lanes, consecutive elements of a row
  int e0 = 0;   // elements of a row written so far
  auto flush = [&](int used) {
    staged_wave_sync();
    const int n = used * W;
    for (int e = lane; e < rows_here * n; e += 64) {
      const int r = e / n, j = e - r * n;
      out[(int64_t)r * SW + e0 + j] = tile[r * P + j];
    }
    e0 += n;
    staged_wave_sync();   // the next stage overwrites the tile
  };

  ACC acc[KMAX];
  init_acc(acc, a);
  KArgs fa = a;   // finish_row's view: this lane's tile row is its `out`, row 0
  int s = 0, slot = 0;
  int next_end = a.st_ends[0];

  int32_t pre[kStTC];
  load_chunk(t_first, pre);
  store_chunk(slice, pre);
  staged_wave_sync();
  int buf = 0;
  for (int t0 = t_first; t0 < t_last; t0 += kStTC, buf ^= 1) {
    const int tc = t_last - t0 < kStTC ? t_last - t0 : kStTC;
    const bool more = t0 + kStTC < t_last;
    if (more) load_chunk(t0 + kStTC, pre);   // in flight while this chunk's chain runs
    const int32_t* sl = slice + buf * 64 * kStPitch + lane * kStPitch;
    for (int j0 = 0; j0 < tc; j0 += kGather) {
      ACC v[kGather][VEC ? KMAX : 1] = {};
#pragma unroll
      for (int b = 0; b < kGather; ++b) {
        if (j0 + b >= tc) continue;   // uniform
        const int t = t0 + j0 + b;
        const int64_t lb = a.leaf_base[t];
        const uint32_t n = (uint32_t)(a.leaf_base[t + 1] - lb);
        uint32_t id = (uint32_t)sl[j0 + b];
        id = id < n ? id : 0u;   // pass 1 reports none outside its tree
        const ACC* p = leaves + (lb + id) * LW;
        if (VEC) {
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < LW) v[b][k] = p[k];
        } else {
          v[b][0] = p[0];
        }
      }
#pragma unroll
      for (int b = 0; b < kGather; ++b) {
        if (j0 + b >= tc) continue;
        const int t = t0 + j0 + b;
        if (VEC) {   // add_leaf's vector form, the values already in registers
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < LW) acc[k] += v[b][k];
        } else if (K == 1) acc[0] += v[b][0];
        else add_leaf<ACC, KMAX>(acc, v[b], 0, 1, a.tree_group[t]);
        if (t + 1 == next_end) {   // uniform: a stage ends behind tree t
          fa.out = tile + lane * P + slot * W;
          finish_row<ACC, KMAX>(acc, fa, 0);
          ++s;
          next_end = s < S ? a.st_ends[s] : -1;
          if (++slot == slots) {
            flush(slot);
            slot = 0;
          }
        }
      }
    }
    if (more) {
      store_chunk(slice + (buf ^ 1) * 64 * kStPitch, pre);
      staged_wave_sync();
    }
  }
  if (slot > 0) flush(slot);
}

}  // namespace ti
