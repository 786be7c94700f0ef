// Ranks of given item ids inside per-row candidate lists, by counting (include/rsx.h rsx_rank_count_lists).  Row u is one user's
// candidate list as rsx_din_retrieve_candidates wrote it and rsx_predict_din_rank scored it: n columns of which the first
// n_valid[u] are live, cand_pos ascending over them, cand_id the item ids beside it, scores the probabilities.  For slot t with
// tgt_id[u, t] > 0 the kernel finds c, the LOWEST live column whose id is the target's, and writes the column's score bits, its
// catalogue position, and the number of live columns j with tk_key(scores[u, j], j) > tk_key(scores[u, c], c): the 0-based index
// at which that candidate stands in the list rsx_topk_rows_counted would select.  serving.Predictor.evaluate_two_stage runs it
// behind the retrieval and the rank launch of a block of users.
//
// The order is topk.hip's (topk_device.h tk_key: a higher score first, equal scores -- -0.0 == +0.0 -- by the lower column, NaN
// last), reused, not restated.  Keys are unique per (row, column), so the target's own column compares equal and is never counted.
// cand_pos ascends with the column, so "the lower column" is "the lower catalogue position": recommend_two_stage's order.
//
// GRID: one workgroup of 256 threads per row, two passes over the row's live columns (n is a candidate capacity: a few
// thousand at the most, and a block of users is a handful of rows beside the rank launch that produced the scores).
//   pass 1: every live column's id against the T target ids (registers); a match does an integer LDS atomicMin of the column
//           into the slot's word.  A minimum does not depend on the order of the threads.
//   pass 2: rank_count.hip's count -- the T keys and T counters in registers, n x T 64-bit compares, __shfl_down wave reduction,
//           one LDS word per (wave, slot), thread t sums the four.
// Every output slot [U, T] is WRITTEN (found or not), so there is no zeroing launch, no global atomic, no workspace, and no
// grid-wide step.  Columns at and beyond n_valid[u] are never read: not their ids, not their scores.  Compiled for T capacities
// 1, 8 and 32 like rank_count.hip; slots past T hold the id 0 (matches nothing) and the key ~0 (no score exceeds it).
#include "topk_device.h"

namespace {

constexpr int RL_THREADS = 256;          // 4 waves
constexpr int RL_TMAX = 32;              // largest T
constexpr int RL_NOCOL = 0x7fffffff;     // above every column
constexpr unsigned long long RL_NOKEY = ~0ull;      // above every tk_key (the largest image, +inf's, is 0xff800000)

struct RankListsArgs {
  const float* scores;
  const int32_t* cand_id;
  const int32_t* cand_pos;
  const int32_t* n_valid;
  const int32_t* tgt_id;
  int32_t* out_count;
  int32_t* out_pos;
  float* out_score;
  int ld, n, T;
};

template <int TC>
__global__ __launch_bounds__(RL_THREADS) void rank_count_lists_k(const RankListsArgs p) {
  __shared__ int col[RL_TMAX];
  __shared__ unsigned long long tkey[RL_TMAX];
  __shared__ int part[RL_THREADS / 64][RL_TMAX];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.T, n = p.n;
  const size_t row = blockIdx.x;
  const float* sc = p.scores + row * (size_t)p.ld;
  const int32_t* id = p.cand_id + row * (size_t)n;
  int nv = p.n_valid[row];
  nv = nv < 0 ? 0 : (nv > n ? n : nv);                                 // a count nobody clamped must not index out of the row

  if (tid < TC) col[tid] = RL_NOCOL;
  int tg[TC];
#pragma unroll
  for (int t = 0; t < TC; ++t) {
    const int v = t < T ? p.tgt_id[row * (size_t)T + t] : 0;
    tg[t] = v > 0 ? v : 0;
  }
  __syncthreads();

  // pass 1: the lowest live column of every target id
  for (int j = tid; j < nv; j += RL_THREADS) {
    const int v = id[j];
    if (v <= 0) continue;                                              // (item 0 is no target: tg holds 0 for "no target")
#pragma unroll
    for (int t = 0; t < TC; ++t)
      if (v == tg[t]) atomicMin(&col[t], j);
  }
  __syncthreads();

  if (tid < TC) {
    const int c = col[tid];
    const bool found = c != RL_NOCOL;
    tkey[tid] = found ? tk_key(sc[c], c) : RL_NOKEY;
    if (tid < T) {
      p.out_pos[row * (size_t)T + tid] = found ? p.cand_pos[row * (size_t)n + c] : -1;
      p.out_score[row * (size_t)T + tid] = found ? sc[c] : __uint_as_float(0x7fc00000u);
    }
  }
  __syncthreads();

  // pass 2: the live columns that precede each target
  unsigned long long tk[TC];
  int cnt[TC];
#pragma unroll
  for (int t = 0; t < TC; ++t) {
    tk[t] = tkey[t];
    cnt[t] = 0;
  }
  for (int j = tid; j < nv; j += RL_THREADS) {
    const unsigned long long key = tk_key(sc[j], j);
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
  if (tid < T) {
    int s = 0;
    for (int w = 0; w < RL_THREADS / 64; ++w) s += part[w][tid];
    p.out_count[row * (size_t)T + tid] = tkey[tid] != RL_NOKEY ? s : -1;
  }
}

inline bool rank_lists_envelope(int n, int T) { return n >= 1 && T >= 1 && T <= RL_TMAX; }

}  // namespace

extern "C" int rsx_rank_count_lists_supported(int n, int T) { return rank_lists_envelope(n, T) ? 1 : 0; }

extern "C" int rsx_rank_count_lists(const float* scores, int ld, const int32_t* cand_id, const int32_t* cand_pos,
                                    const int32_t* n_valid, const int32_t* tgt_id, int T, int32_t* out_count, int32_t* out_pos,
                                    float* out_score, int U, int n, rsx_stream_t stream) {
  if (!scores || !cand_id || !cand_pos || !n_valid || !tgt_id || !out_count || !out_pos || !out_score || U <= 0 || n <= 0 ||
      T <= 0 || ld < n)
    return RSX_EINVAL;
  if (!rank_lists_envelope(n, T)) return RSX_EUNSUPPORTED;
  RankListsArgs p;
  p.scores = scores; p.cand_id = cand_id; p.cand_pos = cand_pos; p.n_valid = n_valid; p.tgt_id = tgt_id;
  p.out_count = out_count; p.out_pos = out_pos; p.out_score = out_score;
  p.ld = ld; p.n = n; p.T = T;
  const dim3 grid((unsigned)U), block(RL_THREADS);
  hipStream_t s = rsx_s(stream);
  if (T <= 1) RSX_LAUNCH(rank_count_lists_k<1>, grid, block, 0, s, p);
  else if (T <= 8) RSX_LAUNCH(rank_count_lists_k<8>, grid, block, 0, s, p);
  else RSX_LAUNCH(rank_count_lists_k<RL_TMAX>, grid, block, 0, s, p);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
