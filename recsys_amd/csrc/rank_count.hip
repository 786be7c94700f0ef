// Ranks of given targets among rows of fp32 scores, by counting (include/rsx.h rsx_rank_count_rows): for row u and slot t,
// count[u, t] += the number of columns j < n that are not excluded for the row and whose key tk_key(scores[u, j],
// first_index + j) is larger than the target's key tk_key(tgt_score[u, t], tgt_pos[u, t]).  serving.Predictor.evaluate_recommend
// runs it behind rsx_predict_din_rank_shared over every chunk of the resident catalogue: the host zeroes `count` once, and after
// the last chunk count[u, t] IS the 0-based rank of the held-out item in the list `recommend` would return.
//
// The order is topk.hip's (topk_device.h tk_key: a higher score first, equal scores -- -0.0 == +0.0 -- by the lower index, NaN
// last) and the exclusion is topk_excl.hip's (tk_excl_sort / tk_excluded: the row's E ids rank-sorted into LDS, every column's
// id looked up by binary search), both reused, not restated.  Keys are unique per (row, index), so the target's own column
// compares equal and is never counted, and a copy of it at a higher position has a smaller key.
//
// GRID: one workgroup of 256 threads per (row, slice of 512 columns) -- a row is NOT bound to one workgroup: a 4 096-column chunk
// of one user is 8 workgroups, the 63 001-item catalogue of 16 users in chunks of 4 096 is 128 per launch.  Every workgroup sorts
// its row's exclusion list itself (E <= 256: E compares per entry, 1 KB of LDS), which is cheaper than a second launch or a
// workspace that would hold the sorted lists.
//
// COST OF T: every kept score is compared against ALL T target keys (n x T 64-bit compares), the keys held in registers (read
// once from LDS, where tid < T built them) and the counters in registers as well.  The alternative -- sort the T keys once and
// bucket each score by binary search, then a suffix sum over the buckets -- saves compares only for large T, needs indexed
// (so LDS or scratch) counters, and T <= 32: at T = 32 a 4 096-column chunk is 131 072 compares per row, small beside the rank
// launch that produced the scores.  The kernel is compiled for T capacities 1, 8 and 32 so a single held-out item does not pay
// for 32; slots past T hold the key ~0, which no score exceeds.
//
// ACCUMULATION: per-thread int counters -> __shfl_down wave reduction -> one LDS word per (wave, slot) -> thread t sums the four
// and issues ONE integer atomicAdd per (workgroup, slot) into count (none when the sum is 0).  Integer sums do not depend on
// the order of the adds: deterministic.  No floating-point atomics, no workspace, no grid-wide step.
#include "topk_device.h"

namespace {

constexpr int RC_THREADS = 256;          // 4 waves
constexpr int RC_COLS = 512;             // columns of a workgroup's slice
constexpr int RC_TMAX = 32;              // largest T
constexpr unsigned long long RC_NOKEY = ~0ull;      // above every tk_key (the largest image, +inf's, is 0xff800000)

struct RankCountArgs {
  const float* scores;
  const int32_t* cand_id;
  const int32_t* excl;
  const float* tgt_score;
  const int32_t* tgt_pos;
  int32_t* count;
  int ld, n, first, E, T, slices;
};

template <int TC>
__global__ __launch_bounds__(RC_THREADS) void rank_count_rows_k(const RankCountArgs p) {
  __shared__ int raw[TK_EMAX], exs[TK_EMAX];
  __shared__ unsigned long long tkey[RC_TMAX];
  __shared__ int part[RC_THREADS / 64][RC_TMAX];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = p.E, T = p.T;
  const size_t row = blockIdx.x / (unsigned)p.slices;
  const int j0 = (int)(blockIdx.x % (unsigned)p.slices) * RC_COLS;
  const int j1 = j0 + RC_COLS < p.n ? j0 + RC_COLS : p.n;
  const float* sc = p.scores + row * (size_t)p.ld;

  if (tid < TC) {
    unsigned long long key = RC_NOKEY;
    if (tid < T) {
      const int pos = p.tgt_pos[row * (size_t)T + tid];
      if (pos >= 0) key = tk_key(p.tgt_score[row * (size_t)T + tid], pos);
    }
    tkey[tid] = key;
  }
  if (E > 0) tk_excl_sort(p.excl + row * (size_t)E, E, raw, exs, tid, RC_THREADS);
  __syncthreads();

  unsigned long long tk[TC];
  int cnt[TC];
#pragma unroll
  for (int t = 0; t < TC; ++t) {
    tk[t] = tkey[t];
    cnt[t] = 0;
  }
  for (int j = j0 + tid; j < j1; j += RC_THREADS) {
    if (E > 0 && tk_excluded(exs, E, p.cand_id[j])) continue;
    const unsigned long long key = tk_key(sc[j], p.first + j);
#pragma unroll
    for (int t = 0; t < TC; ++t) cnt[t] += key > tk[t] ? 1 : 0;
  }
#pragma unroll
  for (int t = 0; t < TC; ++t) {
    int v = cnt[t];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) part[wave][t] = v;
  }
  __syncthreads();
  if (tid < T && tkey[tid] != RC_NOKEY) {                              // a slot with tgt_pos < 0 is left untouched
    int s = 0;
    for (int w = 0; w < RC_THREADS / 64; ++w) s += part[w][tid];
    if (s) atomicAdd(&p.count[row * (size_t)T + tid], s);
  }
}

inline bool rank_count_envelope(int n, int T, int E) { return n >= 1 && T >= 1 && T <= RC_TMAX && E >= 0 && E <= TK_EMAX; }

}  // namespace

extern "C" int rsx_rank_count_rows_supported(int n, int T, int E) { return rank_count_envelope(n, T, E) ? 1 : 0; }

extern "C" int rsx_rank_count_rows(const float* scores, int ld, const int32_t* cand_id, int first_index, const int32_t* excl, int E,
                                   const float* tgt_score, const int32_t* tgt_pos, int T, int32_t* count, int U, int n,
                                   rsx_stream_t stream) {
  if (!scores || !cand_id || !tgt_score || !tgt_pos || !count || U <= 0 || n <= 0 || T <= 0 || ld < n || E < 0 || first_index < 0)
    return RSX_EINVAL;
  if (E > 0 && !excl) return RSX_EINVAL;
  if (!rank_count_envelope(n, T, E) || (long long)first_index + n >= 2147483647ll) return RSX_EUNSUPPORTED;
  const int slices = (n + RC_COLS - 1) / RC_COLS;
  if ((long long)U * slices > 2147483647ll) return RSX_EUNSUPPORTED;
  RankCountArgs p;
  p.scores = scores; p.cand_id = cand_id; p.excl = excl; p.tgt_score = tgt_score; p.tgt_pos = tgt_pos; p.count = count;
  p.ld = ld; p.n = n; p.first = first_index; p.E = E; p.T = T; p.slices = slices;
  const dim3 grid((unsigned)U * (unsigned)slices), block(RC_THREADS);
  hipStream_t s = rsx_s(stream);
  if (T <= 1) RSX_LAUNCH(rank_count_rows_k<1>, grid, block, 0, s, p);
  else if (T <= 8) RSX_LAUNCH(rank_count_rows_k<8>, grid, block, 0, s, p);
  else RSX_LAUNCH(rank_count_rows_k<RC_TMAX>, grid, block, 0, s, p);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
