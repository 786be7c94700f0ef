// Exact, tie-aware ROC AUC on gfx950 (include/rsx.h rsx_auc_exact_*): the rank statistic the reference's serving client reports
// (sklearn.metrics.roc_auc_score, deepfm/grpc_client.py:84) for the probabilities the eval_metric_ops of fm/fm.py:150-153 see --
// beside, never instead of, the 200-threshold tf.metrics.auc of csrc/metrics.hip.
//
// THE CONTRACT, in integers.  Whether an example (fp32 p, label y) is positive and whether it is valid (0 <= p <= 1) is the
// example rule of csrc/eval_device.h, stated there once for all the opt-in eval metrics.  A valid example is ONE 32-bit key
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
#include "eval_device.h"      // the example rule and the append kernel, the workgroup scans, the key predicates, the tile load

namespace {
constexpr int AX_PASSES = 4;

// ---- append: ev_append_k<uint32_t, false> of csrc/eval_device.h; sort: csrc/auc_sort_device.h ---------------------------------
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

typedef EvTile<uint32_t> AxTile;

__global__ __launch_bounds__(AX_T) void ax_counts_k(const AxRed a) {
  __shared__ uint32_t l32[AX_W], lmax[AX_W], lsum[AX_W];
  const int tid = threadIdx.x;
  unsigned long long positives = 0ull;                    // thread 0: over this workgroup's tiles
  for (int t = blockIdx.x; t < a.nT; t += gridDim.x) {
    AxTile s;
    ev_load_tile(a.keys, a.n, t, l32, s);
    uint32_t run = s.excl, lh = 0u, pc = 0u;
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      if (ev_shead(s.k[k], k == 0 ? s.prev : s.k[k - 1])) lh = run + 1u;
      run += ev_neg(s.k[k]) ? 1u : 0u;
      pc += ev_pos(s.k[k]) ? 1u : 0u;
    }
    const uint32_t mh = ev_block_reduce<true, AX_W>(lh, lmax);     // (the next tile's load holds the barriers that free the arrays)
    const uint32_t ptot = ev_block_reduce<false, AX_W>(pc, lsum);
    if (tid == 0) {
      a.tneg[t] = s.total;
      a.thead[t] = mh;
      positives += ptot;
    }
  }
  if (tid == 0 && positives) atomicAdd(&a.out[1], positives);
}

// ONE workgroup: tneg -> negatives in front of every tile; thead -> c at the last head in front of it (the running maximum of
// the tiles' head values: c never decreases, so "the last" is "the largest"; 0 when there is none, which only the first tile
// sees, whose first key is a head itself).  Then out[2] = N and out[3] = n - P - N.
__global__ __launch_bounds__(AX_T) void ax_tile_scan_k(const AxRed a) {
  __shared__ uint32_t l32[AX_W];
  uint32_t N = 0u, hmax = 0u;                             // carried over the rounds of AX_T tiles: both scans in one sweep
  for (int t0 = 0; t0 < a.nT; t0 += AX_T) {
    const int t = t0 + (int)threadIdx.x;
    const uint32_t c = t < a.nT ? a.tneg[t] : 0u, l = t < a.nT ? a.thead[t] : 0u;
    uint32_t tot, mx;
    const uint32_t base = N + ev_block_excl<false, AX_W>(c, l32, tot);
    const uint32_t g = l ? base + l - 1u : 0u;            // global c at the tile's last head
    const uint32_t hin = ev_op<true>(hmax, ev_block_excl<true, AX_W>(g, l32, mx));
    if (t < a.nT) {
      a.tneg[t] = base;
      a.thead[t] = hin;
    }
    N += tot;
    hmax = ev_op<true>(hmax, mx);
  }
  if (threadIdx.x == 0) {
    const unsigned long long P = a.out[1];
    a.out[2] = N;
    a.out[3] = (unsigned long long)a.n - P - N;
  }
}

__global__ __launch_bounds__(AX_T) void ax_u2_k(const AxRed a) {
  __shared__ uint32_t l32[AX_W];
  __shared__ unsigned long long l64[AX_W];
  unsigned long long acc = 0ull;
  for (int t = blockIdx.x; t < a.nT; t += gridDim.x) {
    AxTile s;
    ev_load_tile(a.keys, a.n, t, l32, s);
    uint32_t c[AX_IPL];
    bool head[AX_IPL];
    uint32_t run = a.tneg[t] + s.excl, hv = 0u;           // hv: c at my last head (0: none -- the identity of the maximum)
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      c[k] = run;
      head[k] = ev_shead(s.k[k], k == 0 ? s.prev : s.k[k - 1]);
      if (head[k]) hv = run;
      run += ev_neg(s.k[k]) ? 1u : 0u;
    }
    uint32_t m;
    uint32_t cur = ev_op<true>(ev_block_excl<true, AX_W>(hv, l32, m), a.thead[t]);
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      if (head[k]) cur = c[k];
      if (ev_pos(s.k[k])) acc += (unsigned long long)c[k] + (unsigned long long)cur;
    }
  }
  const unsigned long long sum = ev_block_reduce<false, AX_W>(acc, l64);
  if (threadIdx.x == 0 && sum) atomicAdd(&a.out[0], sum);
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
  ev_append<uint32_t, false>(prob, labels, nullptr, 1, n, 0u, keys_at_offset, counters, rsx_s(stream));
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
