// The multi-workgroup stable LSD radix sort of the AUC metrics, templated on the key type: csrc/auc_exact.hip sorts 32-bit keys
// (4 passes), csrc/auc_group.hip 64-bit keys (4 + ceil(group_bits / 8) passes over the low 32 + group_bits bits).  8-bit digits;
// per pass { histogram per 4096-key tile ; scan (digit-major, tile-minor) ; stable scatter }, as csrc/sort_large.hip does for ids.
// The padding key (all ones) carries the digit 0xFF in every pass and is larger than every valid key in the sorted bits (bit 31
// of a valid key is clear), so it ends up last.  Workgroups meet only at kernel boundaries and in integer atomics; grids are
// bounded (AX_MAX_GRID workgroups stride over the tiles).
//
// Ties.  Histogram atomics of equal scores would all hit one address (csrc/topk.hip's header has the price: 2x at 4 096 equal
// keys).  Here a wave first matches its lanes' digits with ballots -- the scatter needs that mask for the stable rank anyway --
// and ONE lane per distinct digit adds the lane count: 64 equal keys cost one atomic, a wave of distinct ones 64 conflict-free ones.
#pragma once
#include "rsx_common.h"
#include "sort_device.h"      // rsx_match_digit

namespace {
constexpr int AX_TILE = 4096;           // keys per workgroup tile
constexpr int AX_T = 1024;              // threads: 16 waves x 4 items of 64 keys each (wave-major order)
constexpr int AX_W = AX_T / 64;
constexpr int AX_IPL = AX_TILE / AX_T;  // items per lane
constexpr int AX_BINS = 256;
constexpr int AX_MAX_GRID = 1024;
constexpr int64_t AX_MAX_N = 1ll << 27;

template <typename K>
struct AxSort {
  const K* src;
  K* dst;
  uint32_t* hist;      // [AX_BINS, nT]
  uint32_t* dtot;      // [AX_BINS] of this pass
  int n, nT, shift;
};

// lanes of this wave that hold a key (ok) with my digit; lanes past n match among themselves only
__device__ __forceinline__ uint64_t ax_match(uint32_t d, bool ok) {
  uint64_t m = __ballot(ok);
  m = ok ? m : ~m;
  return m & rsx_match_digit(d, 8);
}

template <typename K>
__global__ __launch_bounds__(AX_T) void ax_hist_k(const AxSort<K> a) {
  __shared__ uint32_t h[AX_BINS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  if (tid < AX_BINS) h[tid] = 0u;
  uint32_t tot = 0u;                                      // thread d < 256: this workgroup's keys of digit d, over its tiles
  __syncthreads();
  for (int t = blockIdx.x; t < a.nT; t += gridDim.x) {
    K key[AX_IPL];
    bool ok[AX_IPL];
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      const int i = t * AX_TILE + w * (AX_IPL * 64) + k * 64 + lane;
      ok[k] = i < a.n;
      key[k] = ok[k] ? a.src[i] : ~(K)0;
    }
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      const uint32_t d = (uint32_t)(key[k] >> a.shift) & 255u;
      const uint64_t m = ax_match(d, ok[k]);
      if (ok[k] && (m & lt) == 0ull) atomicAdd(&h[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (tid < AX_BINS) {
      const uint32_t c = h[tid];
      a.hist[(size_t)tid * a.nT + t] = c;
      tot += c;
      h[tid] = 0u;
    }
    __syncthreads();
  }
  if (tid < AX_BINS && tot) atomicAdd(&a.dtot[tid], tot);
}

// grid AX_BINS / 4, block 256: one wave per digit.  Its base is the sum of the smaller digits' totals; its tiles are scanned 64 at
// a time with lane shuffles (the loads of successive rounds do not depend on each other), in place.
template <typename K>
__global__ __launch_bounds__(256) void ax_scan_k(const AxSort<K> a) {
  const int d = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  uint32_t base = 0u;
#pragma unroll
  for (int k = 0; k < AX_BINS / 64; ++k) {
    const int dd = lane + 64 * k;
    const uint32_t v = a.dtot[dd];
    base += dd < d ? v : 0u;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) base += (uint32_t)__shfl_xor((int)base, m);
  uint32_t* h = a.hist + (size_t)d * a.nT;
  for (int t0 = 0; t0 < a.nT; t0 += 64) {
    const int t = t0 + lane;
    const uint32_t c = t < a.nT ? h[t] : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, s);
      if (lane >= s) incl += o;
    }
    if (t < a.nT) h[t] = base + incl - c;
    base += (uint32_t)__shfl((int)incl, 63);
  }
}

// Stable scatter of one tile at a time.  Position = global offset of (digit, tile) + keys of the same digit in earlier waves of
// the tile + rank among the equal-digit lanes below me (ballots: stable, no atomics in the ranking).
template <typename K>
__global__ __launch_bounds__(AX_T) void ax_scatter_k(const AxSort<K> a) {
  __shared__ uint32_t cnt[AX_W][AX_BINS];                 // 16 KB
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  for (int t = blockIdx.x; t < a.nT; t += gridDim.x) {
    for (int i = tid; i < AX_W * AX_BINS; i += AX_T) (&cnt[0][0])[i] = 0u;
    __syncthreads();
    K key[AX_IPL];
    uint64_t msk[AX_IPL];
    bool ok[AX_IPL];
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      const int i = t * AX_TILE + w * (AX_IPL * 64) + k * 64 + lane;
      ok[k] = i < a.n;
      key[k] = ok[k] ? a.src[i] : ~(K)0;
    }
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      const uint32_t d = (uint32_t)(key[k] >> a.shift) & 255u;
      msk[k] = ax_match(d, ok[k]);
      if (ok[k] && (msk[k] & lt) == 0ull) atomicAdd(&cnt[w][d], (uint32_t)__popcll(msk[k]));
    }
    __syncthreads();
    if (tid < AX_BINS) {
      uint32_t run = a.hist[(size_t)tid * a.nT + t];
#pragma unroll
      for (int ww = 0; ww < AX_W; ++ww) {
        const uint32_t c = cnt[ww][tid];
        cnt[ww][tid] = run;
        run += c;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      const uint32_t d = (uint32_t)(key[k] >> a.shift) & 255u;
      const uint32_t old = cnt[w][d];
      const int r = __popcll(msk[k] & lt);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (ok[k] && r == 0) cnt[w][d] = old + (uint32_t)__popcll(msk[k]);
      if (ok[k]) a.dst[old + r] = key[k];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __syncthreads();                                      // cnt is zeroed again for the next tile
  }
}

template <typename K>
__global__ __launch_bounds__(AX_T) void ax_copy_k(const K* __restrict__ src, K* __restrict__ dst, int n) {
  for (int i = blockIdx.x * AX_T + threadIdx.x; i < n; i += gridDim.x * AX_T) dst[i] = src[i];
}

inline size_t ax_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t ax_tiles(int64_t n) { return (size_t)((n + AX_TILE - 1) / AX_TILE); }
inline unsigned ax_grid(int nT) { return (unsigned)(nT < AX_MAX_GRID ? nT : AX_MAX_GRID); }

// `passes` passes over the digits 0 .. passes - 1 of keys[0 .. n), n > 0; alt: n keys, hist: [AX_BINS, nT], dtot: [passes, AX_BINS]
// zeroed by the caller.  The sorted keys end in `keys`: an odd pass count starts from a copy in `alt`.
template <typename K>
inline void ax_sort_passes(K* keys, K* alt, uint32_t* hist, uint32_t* dtot, int n, int nT, int passes, hipStream_t st) {
  const unsigned grid = ax_grid(nT);
  K* buf[2] = {keys, alt};
  int cur = 0;
  if (passes & 1) {
    RSX_LAUNCH((ax_copy_k<K>), dim3(grid), dim3(AX_T), 0, st, keys, alt, n);
    cur = 1;
  }
  for (int pass = 0; pass < passes; ++pass) {
    AxSort<K> a;
    a.src = buf[cur];
    a.dst = buf[cur ^ 1];
    a.hist = hist;
    a.dtot = dtot + pass * AX_BINS;
    a.n = n; a.nT = nT; a.shift = 8 * pass;
    RSX_LAUNCH((ax_hist_k<K>), dim3(grid), dim3(AX_T), 0, st, a);
    RSX_LAUNCH((ax_scan_k<K>), dim3(AX_BINS / 4), dim3(256), 0, st, a);
    RSX_LAUNCH((ax_scatter_k<K>), dim3(grid), dim3(AX_T), 0, st, a);
    cur ^= 1;
  }
}
}  // namespace
