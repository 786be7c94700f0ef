// What the opt-in eval metrics share on the device: csrc/auc_exact.hip, csrc/auc_group.hip, csrc/calibration.hip and
// csrc/calibration_map.hip (csrc/metrics.hip, the 200-threshold AUC, has a rule of its own and takes nothing from here).
//
// THE EXAMPLE RULE, stated here and nowhere else.  An example is (fp32 p, label y).  u = bits(p), with -0.0 taken as +0.0.  It is
// VALID when u <= 0x3F800000 -- 0 <= p <= 1: as unsigned integers the negatives, NaN, the infinities and every p > 1 compare above
// the pattern of 1.0 -- and POSITIVE when y > 0.5f.  Its fixed-point probability is q = uint64(double(p) * 2^32): the product is
// exact in fp64, the conversion truncates, q <= 2^32.  A group id g is valid under a limit when (uint32_t)g < limit (a negative id
// compares above every limit <= 2^31).  metrics.example_bits_host / calibration_q_host are the same rule in numpy.
//
// Then: one invalid-count flush, one append kernel for both key widths, the workgroup scans and reductions (sum or maximum, any
// unsigned T, any wave count), the key predicates and the tile load of the reductions over sorted keys.
#pragma once
#include "rsx_common.h"
#include "auc_sort_device.h"  // AX_TILE / AX_T / AX_W / AX_IPL: a tile of the reductions is a tile of the sort

namespace {
typedef unsigned long long ull;

// ---- the example rule ---------------------------------------------------------------------------------------------------------
struct EvExample {
  uint32_t u;          // bits(p), -0.0 as +0.0
  bool pos, valid;
};

__device__ __forceinline__ EvExample ev_example(float p, float y) {
  uint32_t u = __float_as_uint(p);
  if (u == 0x80000000u) u = 0u;
  return {u, y > 0.5f, u <= 0x3F800000u};
}

__device__ __forceinline__ ull ev_q(uint32_t u) { return (ull)((double)__uint_as_float(u) * 4294967296.0); }

__device__ __forceinline__ bool ev_group_ok(int32_t g, uint32_t limit) { return (uint32_t)g < limit; }

// ---- workgroup scans ----------------------------------------------------------------------------------------------------------
template <bool MAX, typename T>
__device__ __forceinline__ T ev_op(T a, T b) {
  return MAX ? (a > b ? a : b) : a + b;
}

// Exclusive sum or running maximum of v over the workgroup's 64 W threads (unsigned values: the identity of both is 0); total:
// over all threads.  lds: W words.  Ends with every thread past the barrier that makes lds reusable.  (Today every scan runs in a
// 1024-thread kernel, W = AX_W; the 256-thread quantile table needs sums only and takes ev_block_reduce.)
template <bool MAX, int W, typename T>
__device__ __forceinline__ T ev_block_excl(T v, T* lds, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(incl, d);
    if (lane >= d) incl = ev_op<MAX>(incl, o);
  }
  if (lane == 63) lds[w] = incl;
  T ex = __shfl_up(incl, 1);
  if (lane == 0) ex = (T)0;
  __syncthreads();
  T pre = (T)0, tot = (T)0;
#pragma unroll
  for (int ww = 0; ww < W; ++ww) {
    const T x = lds[ww];
    if (ww < w) pre = ev_op<MAX>(pre, x);
    tot = ev_op<MAX>(tot, x);
  }
  __syncthreads();
  total = tot;
  return ev_op<MAX>(pre, ex);
}

// Sum or maximum of v over the workgroup's 64 W threads, returned to thread 0 alone (every other thread gets 0).  ONE
// barrier, and lds (W words) is read behind it: a call site inside a loop has an array of its own, and whatever barrier the loop
// holds elsewhere is what makes the array reusable.
template <bool MAX, int W, typename T>
__device__ __forceinline__ T ev_block_reduce(T v, T* lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = ev_op<MAX>(v, (T)__shfl_xor(v, d));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = (T)0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int ww = 0; ww < W; ++ww) r = ev_op<MAX>(r, lds[ww]);
  }
  return r;
}

// ONE workgroup of 64 W threads: exclusive scan of arr[0 .. nT) in place, of the values pre(t, arr[t]); returns the total.  Thread
// tid handles the tiles t0 + tid, so pre may read what the same thread wrote to another array in an earlier scan of this launch.
template <bool MAX, int W, typename T, typename F>
__device__ __forceinline__ T ev_tiles_scan(T* arr, int nT, T* lds, F pre) {
  T carry = (T)0;
  for (int t0 = 0; t0 < nT; t0 += 64 * W) {
    const int t = t0 + (int)threadIdx.x;
    const T v = t < nT ? pre(t, arr[t]) : (T)0;
    T tot;
    const T ex = ev_block_excl<MAX, W>(v, lds, tot);
    if (t < nT) arr[t] = ev_op<MAX>(carry, ex);
    carry = ev_op<MAX>(carry, tot);
  }
  return carry;
}

// The invalid count of a launch.  Per example: wave_bad += ev_count_invalid(!valid), called by every lane that holds an example
// (before any lane leaves the iteration): the ballot counts the wave's invalid examples of that iteration, so no shuffle is needed
// at the end.  A lane holds the wave's whole count only if it took part in every iteration any lane of its wave took part in.
// LANE 0 does, and it is the one ev_flush_invalid reads: in a grid-stride loop whose index grows with the lane, lane 0 holds the
// wave's smallest i, so it leaves the loop last; lanes with i >= n miss the last iteration's ballot and hold less.  A loop that
// maps indices to lanes differently has to keep that property.
// Then once, from every thread, ev_flush_invalid: one 64-bit atomic per workgroup, and none when the workgroup counted nothing.
// It holds ONE barrier, so LDS atomics issued before it are visible behind it.
__device__ __forceinline__ unsigned int ev_count_invalid(bool bad) { return (unsigned int)__popcll(__ballot(bad)); }

template <int W>
__device__ __forceinline__ void ev_flush_invalid(unsigned int wave_bad, ull* invalid_word) {
  __shared__ unsigned int lds[W];
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = wave_bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int bad = 0u;
#pragma unroll
    for (int ww = 0; ww < W; ++ww) bad += lds[ww];
    if (bad) atomicAdd(invalid_word, (ull)bad);
  }
}

// ---- append: one launch per eval batch ----------------------------------------------------------------------------------------
// K = uint32_t: the key (u << 1) | positive.  K = uint64_t with GROUPS: (uint64(g) << 32) | that key, the group column read
// through its element stride.  An invalid example is the padding key ~K(0), which sorts to the end, and is counted.
constexpr int EV_APPEND_T = 256;
constexpr int EV_APPEND_MAX_GRID = 256;

template <typename K, bool GROUPS>
__global__ __launch_bounds__(EV_APPEND_T) void ev_append_k(const float* __restrict__ prob, const float* __restrict__ labels,
                                                           const int32_t* __restrict__ groups, int64_t gstride, int64_t n,
                                                           uint32_t glimit, K* __restrict__ keys, ull* invalid_word) {
  static_assert(!GROUPS || sizeof(K) == 8, "the group id takes a 64-bit key's upper word");
  unsigned int wave_bad = 0u;
  for (int64_t i = (int64_t)blockIdx.x * EV_APPEND_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * EV_APPEND_T) {
    const EvExample e = ev_example(prob[i], labels[i]);
    bool valid = e.valid;
    K key = (K)((e.u << 1) | (e.pos ? 1u : 0u));
    if constexpr (GROUPS) {
      const int32_t g = groups[i * gstride];
      valid = valid && ev_group_ok(g, glimit);
      key |= (K)(uint32_t)g << 32;
    }
    keys[i] = valid ? key : ~(K)0;
    wave_bad += ev_count_invalid(!valid);
  }
  ev_flush_invalid<EV_APPEND_T / 64>(wave_bad, invalid_word);
}

template <typename K, bool GROUPS>
inline void ev_append(const float* prob, const float* labels, const int32_t* groups, int64_t gstride, int64_t n, uint32_t glimit,
                      K* keys, uint64_t* invalid_word, hipStream_t st) {
  int64_t blocks = (n + EV_APPEND_T - 1) / EV_APPEND_T;
  if (blocks > EV_APPEND_MAX_GRID) blocks = EV_APPEND_MAX_GRID;
  RSX_LAUNCH((ev_append_k<K, GROUPS>), dim3((unsigned)blocks), dim3(EV_APPEND_T), 0, st, prob, labels, groups, gstride, n, glimit,
             keys, reinterpret_cast<ull*>(invalid_word));
}

// ---- sorted keys: predicates and the tile load --------------------------------------------------------------------------------
// K is uint32_t (score, label) or uint64_t (group, score, label); a head is a key whose field differs from its predecessor's.
template <typename K>
__device__ __forceinline__ bool ev_valid(K k) { return k != ~(K)0; }
template <typename K>
__device__ __forceinline__ bool ev_neg(K k) { return ev_valid(k) && (k & (K)1) == (K)0; }
template <typename K>
__device__ __forceinline__ bool ev_pos(K k) { return ev_valid(k) && (k & (K)1) != (K)0; }
template <typename K>
__device__ __forceinline__ bool ev_shead(K k, K pk) { return ev_valid(k) && (k >> 1) != (pk >> 1); }
__device__ __forceinline__ bool ev_ghead(uint64_t k, uint64_t pk) { return ev_valid(k) && (k >> 32) != (pk >> 32); }
__device__ __forceinline__ bool ev_gtail(uint64_t k, uint64_t nk) { return ev_valid(k) && (k >> 32) != (nk >> 32); }

static_assert(AX_IPL == 4, "a lane's keys are loaded as 16-byte vectors");

template <typename K>
struct EvTile {
  K k[AX_IPL];
  K prev;              // the key in front of k[0] (padding in front of position 0: position 0 is a head)
  uint32_t excl;       // negatives of the tile in front of k[0]
  uint32_t total;      // negatives of the tile
};

// Thread tid of AX_T holds the keys 4 tid .. 4 tid + 3 of tile t (keys is 16-byte aligned); lds: AX_W words, reusable on return.
template <typename K>
__device__ __forceinline__ void ev_load_tile(const K* __restrict__ keys, int n, int t, uint32_t* lds, EvTile<K>& s) {
  const int i0 = t * AX_TILE + (int)threadIdx.x * AX_IPL;
  if (i0 + AX_IPL <= n) {
    constexpr int PER = 16 / (int)sizeof(K);
    const uint4* q = reinterpret_cast<const uint4*>(keys + i0);
#pragma unroll
    for (int v = 0; v < AX_IPL / PER; ++v) {
      const uint4 x = q[v];
      __builtin_memcpy(&s.k[v * PER], &x, 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) s.k[k] = i0 + k < n ? keys[i0 + k] : ~(K)0;
  }
  s.prev = (i0 > 0 && i0 <= n) ? keys[i0 - 1] : ~(K)0;
  uint32_t c = 0u;
#pragma unroll
  for (int k = 0; k < AX_IPL; ++k) c += ev_neg(s.k[k]) ? 1u : 0u;
  s.excl = ev_block_excl<false, AX_W>(c, lds, s.total);
}
}  // namespace
