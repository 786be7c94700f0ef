// Exact, tie-aware ROC AUC on gfx950 (include/rsx.h rsx_auc_exact_*): the rank statistic the reference's serving client reports
// (sklearn.metrics.roc_auc_score, deepfm/grpc_client.py:84) for the probabilities the eval_metric_ops of fm/fm.py:150-153 see --
// beside, never instead of, the 200-threshold tf.metrics.auc of csrc/metrics.hip.
//
// THE CONTRACT, in integers.  An example (fp32 p, label y) is positive when y > 0.5f (metrics.hip's rule) and valid when
// 0 <= p <= 1 (-0.0 counts as +0.0; NaN, infinities, everything else: invalid).  A valid example is ONE 32-bit key
//     (bits(p) << 1) | positive          bits(p) <= 0x3F800000: 31 bits, unsigned key order = score order, and within one score
//                                        the negatives sort in front of the positives; subnormals stay distinct scores
// and an invalid one the padding key 0xFFFFFFFF, which sorts to the end and takes no part.  Over the sorted valid keys let c[i]
// be the number of negatives in front of position i (it never decreases) and h[i] the value of c at the head of i's score group
// (a head: key >> 1 differs from the predecessor's) -- the running maximum of c over the heads up to i.  For a positive at i,
// c[i] counts the negatives with a score <= its own and h[i] those with a strictly smaller one, so
//     U2 = sum over positives of (2 #{smaller negatives} + #{equal negatives}) = sum over positives of (c[i] + h[i])
// and AUC = U2 / (2 P N), a quotient the HOST takes from integers.  Everything here is integer arithmetic: the four words do not
// depend on batch sizes, batch order or the order threads run in.
//
// KERNELS.  append (one launch per eval batch): keys at the slot the host names, the batch's invalid count with one 64-bit
// integer atomic per workgroup.  finalize:
//   zero        digit totals + the output words
//   4 passes x  { histogram per 4096-key tile ; scan (digit-major, tile-minor) ; stable scatter }     8-bit digits over all 32 bits:
//               a stable LSD radix sort as csrc/sort_large.hip does for ids; the padding keys' top digit 0xFF keeps them last; an
//               even number of passes leaves the sorted keys (the same multiset) in the caller's buffer
//   counts      per tile: negatives, positives (one atomic per workgroup), local c at the tile's last head
//   tile scan   ONE workgroup: exclusive sum of the negatives and exclusive running maximum of the head values over the tiles
//   u2          per tile: c and h of every position from the tile's (count, last-head value) pair, the positives' c + h summed
//               in 64 bits, one integer atomic per workgroup
// Every step that needs another workgroup's result is a kernel boundary: no grid barrier, no spin-wait, no look-back chain; inside
// a launch workgroups meet in integer atomics only.  Grids are bounded (AX_MAX_GRID workgroups stride over the tiles).
//
// The sort's kernels live in csrc/auc_sort_device.h (how ties are kept off one histogram address is told there), templated on the
// key type: csrc/auc_group.hip sorts its 64-bit keys with them.
#include "rsx_common.h"
#include "auc_sort_device.h"  // the sort's kernels (templated on the key type; csrc/auc_group.hip sorts 64-bit keys with them)

namespace {
constexpr int AX_PASSES = 4;
constexpr uint32_t AX_PAD = 0xFFFFFFFFu;
constexpr int AP_T = 256;

static_assert(AX_IPL == 4, "the reduction loads a lane's keys as one uint4");

// ---- append ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AP_T) void ax_append_k(const float* __restrict__ prob, const float* __restrict__ labels, int64_t n,
                                                    uint32_t* __restrict__ keys, unsigned long long* counters) {
  __shared__ unsigned int bad;
  if (threadIdx.x == 0) bad = 0u;
  __syncthreads();
  unsigned int mine = 0u;
  for (int64_t i = (int64_t)blockIdx.x * AP_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * AP_T) {
    uint32_t u = __float_as_uint(prob[i]);
    if (u == 0x80000000u) u = 0u;                         // -0.0 is +0.0
    const bool valid = u <= 0x3F800000u;                  // 0 <= p <= 1: negatives, NaN, inf and p > 1 all compare above
    const uint32_t pos = labels[i] > 0.5f ? 1u : 0u;
    keys[i] = valid ? ((u << 1) | pos) : AX_PAD;
    mine += valid ? 0u : 1u;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += (unsigned int)__shfl_xor((int)mine, d);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&bad, mine);
  __syncthreads();
  if (threadIdx.x == 0 && bad) atomicAdd(counters, (unsigned long long)bad);
}

// ---- sort: csrc/auc_sort_device.h ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AX_T) void ax_zero_k(uint32_t* dtot, unsigned long long* out) {
  for (int i = threadIdx.x; i < AX_PASSES * AX_BINS; i += AX_T) dtot[i] = 0u;
  if (threadIdx.x < 4) out[threadIdx.x] = 0ull;
}

// ---- reduction over the sorted keys -------------------------------------------------------------------------------------------
struct AxRed {
  const uint32_t* keys;
  uint32_t* tneg;      // [nT]  counts: negatives of the tile          -> tile scan: negatives in front of the tile
  uint32_t* thead;     // [nT]  counts: 1 + local c at the last head   -> tile scan: c at the last head in front of the tile
  unsigned long long* out;
  int n, nT;
};

struct AxTile {
  uint32_t k[AX_IPL];
  uint32_t prev;       // the key in front of k[0] (padding in front of position 0: position 0 is a head)
  uint32_t excl;       // negatives of the tile in front of k[0]
  uint32_t total;      // negatives of the tile
};

__device__ __forceinline__ bool ax_valid(uint32_t k) { return k != AX_PAD; }
__device__ __forceinline__ bool ax_neg(uint32_t k) { return ax_valid(k) && (k & 1u) == 0u; }
__device__ __forceinline__ bool ax_pos(uint32_t k) { return ax_valid(k) && (k & 1u) != 0u; }
__device__ __forceinline__ bool ax_head(uint32_t k, uint32_t pk) { return ax_valid(k) && (k >> 1) != (pk >> 1); }

// thread tid holds the tile's keys 4 tid .. 4 tid + 3; ends with every thread past the barrier that makes wsum reusable
__device__ __forceinline__ void ax_load_tile(const AxRed& a, int t, uint32_t* wsum, AxTile& s) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i0 = t * AX_TILE + tid * AX_IPL;
  if (i0 + AX_IPL <= a.n) {
    const uint4 q = *reinterpret_cast<const uint4*>(a.keys + i0);
    s.k[0] = q.x; s.k[1] = q.y; s.k[2] = q.z; s.k[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) s.k[k] = i0 + k < a.n ? a.keys[i0 + k] : AX_PAD;
  }
  s.prev = (i0 > 0 && i0 <= a.n) ? a.keys[i0 - 1] : AX_PAD;
  uint32_t c = 0u;
#pragma unroll
  for (int k = 0; k < AX_IPL; ++k) c += ax_neg(s.k[k]) ? 1u : 0u;
  uint32_t incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  uint32_t pre = 0u, tot = 0u;
#pragma unroll
  for (int ww = 0; ww < AX_W; ++ww) {
    const uint32_t v = wsum[ww];
    pre += ww < w ? v : 0u;
    tot += v;
  }
  s.excl = pre + incl - c;
  s.total = tot;
  __syncthreads();
}

__global__ __launch_bounds__(AX_T) void ax_counts_k(const AxRed a) {
  __shared__ uint32_t wsum[AX_W], wmax[AX_W], wpos[AX_W];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long positives = 0ull;                    // thread 0: over this workgroup's tiles
  for (int t = blockIdx.x; t < a.nT; t += gridDim.x) {
    AxTile s;
    ax_load_tile(a, t, wsum, s);
    uint32_t run = s.excl, lh = 0u, pc = 0u;
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      if (ax_head(s.k[k], k == 0 ? s.prev : s.k[k - 1])) lh = run + 1u;
      run += ax_neg(s.k[k]) ? 1u : 0u;
      pc += ax_pos(s.k[k]) ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)lh, d);
      lh = o > lh ? o : lh;
      pc += (uint32_t)__shfl_xor((int)pc, d);
    }
    if (lane == 0) { wmax[w] = lh; wpos[w] = pc; }
    __syncthreads();
    if (tid == 0) {
      uint32_t m = 0u, p = 0u;
#pragma unroll
      for (int ww = 0; ww < AX_W; ++ww) {
        m = wmax[ww] > m ? wmax[ww] : m;
        p += wpos[ww];
      }
      a.tneg[t] = s.total;
      a.thead[t] = m;
      positives += p;
    }
    __syncthreads();
  }
  if (tid == 0 && positives) atomicAdd(&a.out[1], positives);
}

// ONE workgroup: tneg -> negatives in front of every tile; thead -> c at the last head in front of it (the running maximum of
// the tiles' head values: c never decreases, so "the last" is "the largest"; 0 when there is none, which only the first tile
// sees, whose first key is a head itself).  Then out[2] = N and out[3] = n - P - N.
__global__ __launch_bounds__(AX_T) void ax_tile_scan_k(const AxRed a) {
  __shared__ uint32_t ws[AX_W], wm[AX_W];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t carry_sum = 0u, carry_max = 0u;
  for (int t0 = 0; t0 < a.nT; t0 += AX_T) {
    const int t = t0 + tid;
    const uint32_t c = t < a.nT ? a.tneg[t] : 0u;
    const uint32_t l = t < a.nT ? a.thead[t] : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == 63) ws[w] = incl;
    __syncthreads();
    uint32_t pre = 0u, tot = 0u;
#pragma unroll
    for (int ww = 0; ww < AX_W; ++ww) {
      const uint32_t v = ws[ww];
      pre += ww < w ? v : 0u;
      tot += v;
    }
    const uint32_t base = carry_sum + pre + incl - c;
    const uint32_t g = l ? base + l - 1u : 0u;            // global c at the tile's last head
    uint32_t gi = g;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)gi, d);
      if (lane >= d) gi = o > gi ? o : gi;
    }
    if (lane == 63) wm[w] = gi;
    uint32_t ge = (uint32_t)__shfl_up((int)gi, 1);
    if (lane == 0) ge = 0u;
    __syncthreads();
    uint32_t hin = carry_max > ge ? carry_max : ge, mx = carry_max;
#pragma unroll
    for (int ww = 0; ww < AX_W; ++ww) {
      const uint32_t v = wm[ww];
      if (ww < w) hin = v > hin ? v : hin;
      mx = v > mx ? v : mx;
    }
    if (t < a.nT) {
      a.tneg[t] = base;
      a.thead[t] = hin;
    }
    carry_sum += tot;
    carry_max = mx;
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned long long P = a.out[1], N = carry_sum;
    a.out[2] = N;
    a.out[3] = (unsigned long long)a.n - P - N;
  }
}

__global__ __launch_bounds__(AX_T) void ax_u2_k(const AxRed a) {
  __shared__ uint32_t wsum[AX_W], wm[AX_W];
  __shared__ unsigned long long wacc[AX_W];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long acc = 0ull;
  for (int t = blockIdx.x; t < a.nT; t += gridDim.x) {
    AxTile s;
    ax_load_tile(a, t, wsum, s);
    const uint32_t base = a.tneg[t], hin = a.thead[t];
    uint32_t c[AX_IPL];
    bool head[AX_IPL];
    uint32_t run = base + s.excl, hv = 0u;                // hv: c at my last head (0: none -- the identity of the maximum)
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      c[k] = run;
      head[k] = ax_head(s.k[k], k == 0 ? s.prev : s.k[k - 1]);
      if (head[k]) hv = run;
      run += ax_neg(s.k[k]) ? 1u : 0u;
    }
    uint32_t gi = hv;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)gi, d);
      if (lane >= d) gi = o > gi ? o : gi;
    }
    if (lane == 63) wm[w] = gi;
    uint32_t cur = (uint32_t)__shfl_up((int)gi, 1);
    if (lane == 0) cur = 0u;
    __syncthreads();
    cur = hin > cur ? hin : cur;
#pragma unroll
    for (int ww = 0; ww < AX_W; ++ww) {
      const uint32_t v = wm[ww];
      if (ww < w) cur = v > cur ? v : cur;
    }
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      if (head[k]) cur = c[k];
      if (ax_pos(s.k[k])) acc += (unsigned long long)c[k] + (unsigned long long)cur;
    }
    __syncthreads();                                      // wm is written again for the next tile
  }
  uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)hi, d) << 32) | (uint32_t)__shfl_xor((int)lo, d);
    acc += o;
    lo = (uint32_t)acc;
    hi = (uint32_t)(acc >> 32);
  }
  if (lane == 0) wacc[w] = acc;
  __syncthreads();
  if (tid == 0) {
    unsigned long long sum = 0ull;
#pragma unroll
    for (int ww = 0; ww < AX_W; ++ww) sum += wacc[ww];
    if (sum) atomicAdd(&a.out[0], sum);
  }
}

}  // namespace

extern "C" int rsx_auc_exact_tile(void) { return AX_TILE; }

extern "C" int64_t rsx_auc_exact_max_keys(void) { return AX_MAX_N; }

// [second key buffer: 4 n, rounded up to 256] [histogram: 4 * 256 * nT] [digit totals: 4 * 4 * 256] [tile pairs: 2 * 4 * nT]
extern "C" size_t rsx_auc_exact_workspace_bytes(int64_t n) {
  if (n < 0 || n > AX_MAX_N) return 0;
  const size_t nT = ax_tiles(n);
  return ax_align((size_t)n * 4) + (size_t)AX_BINS * nT * 4 + (size_t)AX_PASSES * AX_BINS * 4 + nT * 8;
}

extern "C" int rsx_auc_exact_append(const float* prob, const float* labels, int64_t n, uint32_t* keys_at_offset,
                                    uint64_t* counters, rsx_stream_t stream) {
  if (!prob || !labels || !keys_at_offset || !counters || n < 0 || n > AX_MAX_N) return RSX_EINVAL;
  if (n == 0) return RSX_OK;
  int64_t blocks = (n + AP_T - 1) / AP_T;
  if (blocks > 256) blocks = 256;
  RSX_LAUNCH(ax_append_k, dim3((unsigned)blocks), dim3(AP_T), 0, rsx_s(stream), prob, labels, n, keys_at_offset,
             reinterpret_cast<unsigned long long*>(counters));
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}

extern "C" int rsx_auc_exact_finalize(uint32_t* keys, int64_t n, void* workspace, size_t workspace_bytes, uint64_t* out,
                                      rsx_stream_t stream) {
  if (!keys || !workspace || !out || n < 0 || n > AX_MAX_N) return RSX_EINVAL;
  if (workspace_bytes < rsx_auc_exact_workspace_bytes(n)) return RSX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(keys) & 15u) || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return RSX_EINVAL;
  hipStream_t st = rsx_s(stream);
  const int nT = (int)ax_tiles(n);
  char* ws = static_cast<char*>(workspace);
  uint32_t* alt = reinterpret_cast<uint32_t*>(ws);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + ax_align((size_t)n * 4));
  uint32_t* dtot = hist + (size_t)AX_BINS * nT;
  uint32_t* tneg = dtot + AX_PASSES * AX_BINS;
  uint32_t* thead = tneg + nT;
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  RSX_LAUNCH(ax_zero_k, dim3(1), dim3(AX_T), 0, st, dtot, o);
  if (n == 0) {
    RSX_CHECK_LAUNCH();
    return RSX_OK;
  }
  const unsigned grid = ax_grid(nT);
  ax_sort_passes<uint32_t>(keys, alt, hist, dtot, (int)n, nT, AX_PASSES, st);
  RSX_CHECK_LAUNCH();
  AxRed r;
  r.keys = keys; r.tneg = tneg; r.thead = thead; r.out = o; r.n = (int)n; r.nT = nT;
  RSX_LAUNCH(ax_counts_k, dim3(grid), dim3(AX_T), 0, st, r);
  RSX_LAUNCH(ax_tile_scan_k, dim3(1), dim3(AX_T), 0, st, r);
  RSX_LAUNCH(ax_u2_k, dim3(grid), dim3(AX_T), 0, st, r);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
