// Candidate retrieval for a two-stage DIN recommendation (include/rsx.h rsx_din_retrieve_candidates): per user the union of the
// item-neighbour rows of the history's items, without the excluded ids, as an ascending list of catalogue positions with the
// positions' item and category ids beside it -- the candidate lists rsx_predict_din_rank takes.
// serving.Predictor.recommend_two_stage runs it in front of the rank launch; serving.retrieve_candidates_host is the definition.
//
// ONE workgroup of 1024 threads per user, a bitmap of N bits in LDS (7.9 KB at 63 001 entries):
//   (1) the history's ids become SEEDS: an id in (0, n_item) whose first_pos is a catalogue position; every other slot is 0.
//       The seed ids are rank-sorted in LDS (P <= 128) and the exclusion ids beside them (E <= 256, topk_device.h);
//   (2) one thread per (seed, neighbour slot) sets the neighbour's bit with an integer LDS atomicOr -- a set of bits does not
//       depend on the order threads run in.  A neighbour position outside [0, N) sets nothing;
//   (3) include_seeds: a pass over cat_item sets the bit of every position whose id is a seed id (binary search);
//   (4) a thread owns a run of consecutive bitmap words: it clears the bits whose item id is in the exclusion list (binary
//       search), counts what is left, takes its base from a workgroup prefix sum of the counts (wave scans, then the 16 wave
//       totals) and writes its positions in ascending order; the slots from the count to cap are padded with -1 / 0 / 0.
// No global atomics, no workspace; deterministic.  A count above cap cannot occur when cap >= min(N, P (n + 1)); the kernel
// nevertheless writes no slot at or beyond cap and stores n_cand = min(count, cap).
//
// rsx_din_retrieve_candidates_rules is the same body with RULES compiled in (`if constexpr`: the plain kernel holds nothing of
// it): the user's row of the category bitmap allow[u, :Wg], Wg = ceil(G / 32), is staged in LDS behind the waves' totals in (1),
// and the pass of (4) that clears the excluded bits also clears a position whose cat_cate is outside [0, G) or has a clear bit
// in that row -- before the count, so a disallowed position is neither counted nor written.  The seeds are untouched: a
// history item of a denied category still contributes its neighbours.  LDS: the plain plan + 4 Wg bytes; G <= 65 536 (8 KB)
// keeps the largest plan, N = 2^20, at 142 912 bytes of the 163 840.
#include "topk_device.h"         // tk_excl_sort, tk_excluded, launch_big_lds

namespace {

constexpr int RT_T = 1024, RT_NW = RT_T / 64;
constexpr int RT_NMAX = 1 << 20, RT_PMAX = 128, RT_NBRMAX = 64, RT_EMAX = TK_EMAX;

struct RetrieveArgs {
  const int32_t* hist_item;     // [U, P]
  const int32_t* first_pos;     // [n_item]
  const int32_t* nbr_pos;       // [N, nn]
  const int32_t* nbr_count;     // [N]
  const int32_t* cat_item;      // [N]
  const int32_t* cat_cate;      // [N]
  const int32_t* excl;          // [U, E]
  int32_t* cand_pos;            // [U, cap]
  int32_t* cand_item;
  int32_t* cand_cate;
  int32_t* n_cand;              // [U]
  int P, n_item, N, nn, E, cap, include_seeds;
  int W, wpt;                   // bitmap words; words per thread
};

struct RetrieveRulesArgs : RetrieveArgs {
  const uint32_t* allow;        // [U, Wg]: bit g of row u set = category g is allowed for user u
  int G, Wg;
};

// LDS, in words behind the bitmap [W]: seed ids in history order [128], their first positions [128], the seed ids sorted [128],
// the exclusion ids unsorted [256] and sorted [256], the waves' totals [16] (RULES: the user's allow row [Wg])
template <bool RULES, class Args>
__device__ __forceinline__ void din_retrieve_body(const Args& p, unsigned long long* rt_lds64) {
  unsigned* bm = reinterpret_cast<unsigned*>(rt_lds64);
  int* seed = reinterpret_cast<int*>(bm + p.W);
  int* spos = seed + RT_PMAX;
  int* ssort = spos + RT_PMAX;
  int* eraw = ssort + RT_PMAX;
  int* exs = eraw + RT_EMAX;
  int* wsum = exs + RT_EMAX;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t u = blockIdx.x;
  const int P = p.P, N = p.N, nn = p.nn, E = p.E, cap = p.cap;

  // (1)
  for (int w = tid; w < p.W; w += RT_T) bm[w] = 0u;
  if constexpr (RULES) {
    unsigned* alw = reinterpret_cast<unsigned*>(wsum + RT_NW);
    for (int w = tid; w < p.Wg; w += RT_T) alw[w] = p.allow[u * (size_t)p.Wg + w];
  }
  for (int t = tid; t < P; t += RT_T) {
    const int v = p.hist_item[u * (size_t)P + t];
    int at = -1;
    if (v > 0 && v < p.n_item) at = p.first_pos[v];
    const bool ok = at >= 0 && at < N;
    seed[t] = ok ? v : 0;
    spos[t] = ok ? at : -1;
  }
  __syncthreads();
  for (int t = tid; t < P; t += RT_T) {            // rank sort: a permutation, whatever order the threads run in
    const int v = seed[t];
    int rank = 0;
    for (int j = 0; j < P; ++j) {
      const int o = seed[j];
      rank += (o < v || (o == v && j < t)) ? 1 : 0;
    }
    ssort[rank] = v;
  }
  if (E > 0) tk_excl_sort(p.excl + u * (size_t)E, E, eraw, exs, tid, RT_T);
  __syncthreads();

  // (2)
  for (int t = tid; t < P * nn; t += RT_T) {
    const int s = t / nn, r = t - s * nn;
    const int at = spos[s];
    if (at < 0) continue;
    if (r >= p.nbr_count[at]) continue;
    const int q = p.nbr_pos[(size_t)at * nn + r];
    if (q >= 0 && q < N) atomicOr(&bm[q >> 5], 1u << (q & 31));
  }
  // (3)
  if (p.include_seeds) {
    for (int j = tid; j < N; j += RT_T)
      if (tk_excluded(ssort, P, p.cat_item[j])) atomicOr(&bm[j >> 5], 1u << (j & 31));     // (a positive id of the sorted seeds)
  }
  __syncthreads();

  // (4)
  const int w0 = tid * p.wpt;
  const int w1 = w0 + p.wpt < p.W ? w0 + p.wpt : p.W;
  int mine = 0;
  for (int w = w0; w < w1; ++w) {
    unsigned m = bm[w], keep = m;
    while (m) {
      const int b = __ffs((int)m) - 1;
      m &= m - 1u;
      bool out = E > 0 && tk_excluded(exs, E, p.cat_item[w * 32 + b]);
      if constexpr (RULES) {
        const unsigned* alw = reinterpret_cast<const unsigned*>(wsum + RT_NW);
        const int c = p.cat_cate[w * 32 + b];
        if (c < 0 || c >= p.G) out = true;
        else if (!((alw[c >> 5] >> (c & 31)) & 1u)) out = true;
      }
      if (out) keep &= ~(1u << b);
    }
    bm[w] = keep;
    mine += __popc(keep);
  }
  int inc = mine;                                  // inclusive scan inside the wave
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = inc - mine, total = 0;
  for (int w = 0; w < RT_NW; ++w) {
    const int s = wsum[w];
    base += w < wave ? s : 0;
    total += s;
  }
  int32_t* cp = p.cand_pos + u * (size_t)cap;
  int32_t* ci = p.cand_item + u * (size_t)cap;
  int32_t* cc = p.cand_cate + u * (size_t)cap;
  for (int w = w0; w < w1; ++w) {
    unsigned m = bm[w];
    while (m) {
      const int b = __ffs((int)m) - 1;
      m &= m - 1u;
      if (base < cap) {
        const int at = w * 32 + b;
        cp[base] = at;
        ci[base] = p.cat_item[at];
        cc[base] = p.cat_cate[at];
      }
      ++base;
    }
  }
  const int cnt = total < cap ? total : cap;
  for (int c = cnt + tid; c < cap; c += RT_T) {
    cp[c] = -1;
    ci[c] = 0;
    cc[c] = 0;
  }
  if (tid == 0) p.n_cand[u] = cnt;
}

__global__ __launch_bounds__(RT_T) void din_retrieve_k(const RetrieveArgs p) {
  extern __shared__ unsigned long long rt_lds64[];
  din_retrieve_body<false>(p, rt_lds64);
}

__global__ __launch_bounds__(RT_T) void din_retrieve_rules_k(const RetrieveRulesArgs p) {
  extern __shared__ unsigned long long rt_lds64[];
  din_retrieve_body<true>(p, rt_lds64);
}

constexpr int RT_GMAX = 1 << 16;

inline bool retrieve_envelope(int N, int P, int nn, int E) {
  return N >= 1 && N <= RT_NMAX && P >= 1 && P <= RT_PMAX && nn >= 1 && nn <= RT_NBRMAX && E >= 0 && E <= RT_EMAX;
}

// The checks and the launch of both entries; allow == nullptr: the plain kernel.
inline int retrieve_launch(const int32_t* hist_item, int P, const int32_t* first_pos, int n_item, const int32_t* nbr_pos,
                           const int32_t* nbr_count, int n_nbr, const int32_t* cat_item, const int32_t* cat_cate, int N,
                           const int32_t* excl, int E, int include_seeds, const uint32_t* allow, int G, int32_t* cand_pos,
                           int32_t* cand_item, int32_t* cand_cate, int32_t* n_cand, int cap, int U, rsx_stream_t stream) {
  if (!hist_item || !first_pos || !nbr_pos || !nbr_count || !cat_item || !cat_cate || !cand_pos || !cand_item || !cand_cate ||
      !n_cand || U <= 0 || P <= 0 || n_item <= 0 || n_nbr <= 0 || N <= 0 || E < 0 || cap <= 0)
    return RSX_EINVAL;
  if (E > 0 && !excl) return RSX_EINVAL;
  if (allow && G <= 0) return RSX_EINVAL;
  if (!retrieve_envelope(N, P, n_nbr, E)) return RSX_EUNSUPPORTED;
  if (allow && G > RT_GMAX) return RSX_EUNSUPPORTED;
  RetrieveRulesArgs p;
  p.hist_item = hist_item; p.first_pos = first_pos; p.nbr_pos = nbr_pos; p.nbr_count = nbr_count;
  p.cat_item = cat_item; p.cat_cate = cat_cate; p.excl = excl;
  p.cand_pos = cand_pos; p.cand_item = cand_item; p.cand_cate = cand_cate; p.n_cand = n_cand;
  p.P = P; p.n_item = n_item; p.N = N; p.nn = n_nbr; p.E = E; p.cap = cap; p.include_seeds = include_seeds ? 1 : 0;
  p.W = (N + 31) / 32;
  p.wpt = (p.W + RT_T - 1) / RT_T;
  p.allow = allow; p.G = allow ? G : 0; p.Wg = (p.G + 31) / 32;
  const size_t lds = 4 * ((size_t)p.W + 3 * RT_PMAX + 2 * RT_EMAX + RT_NW + (size_t)p.Wg);
  if (lds > (size_t)PR_MAX_LDS) return RSX_EUNSUPPORTED;
  if (!allow) return launch_big_lds<din_retrieve_k>(static_cast<const RetrieveArgs&>(p), (unsigned)U, RT_T, lds, rsx_s(stream));
  return launch_big_lds<din_retrieve_rules_k>(p, (unsigned)U, RT_T, lds, rsx_s(stream));
}

}  // namespace

extern "C" int rsx_din_retrieve_candidates_supported(int N, int P, int n_nbr, int E) { return retrieve_envelope(N, P, n_nbr, E) ? 1 : 0; }

extern "C" int rsx_din_retrieve_candidates(const int32_t* hist_item, int P, const int32_t* first_pos, int n_item,
                                           const int32_t* nbr_pos, const int32_t* nbr_count, int n_nbr, const int32_t* cat_item,
                                           const int32_t* cat_cate, int N, const int32_t* excl, int E, int include_seeds,
                                           int32_t* cand_pos, int32_t* cand_item, int32_t* cand_cate, int32_t* n_cand, int cap,
                                           int U, rsx_stream_t stream) {
  return retrieve_launch(hist_item, P, first_pos, n_item, nbr_pos, nbr_count, n_nbr, cat_item, cat_cate, N, excl, E, include_seeds,
                         nullptr, 0, cand_pos, cand_item, cand_cate, n_cand, cap, U, stream);
}

extern "C" int rsx_din_retrieve_candidates_rules_supported(int N, int P, int n_nbr, int E, int G) {
  return retrieve_envelope(N, P, n_nbr, E) && G >= 1 && G <= RT_GMAX ? 1 : 0;
}

extern "C" int rsx_din_retrieve_candidates_rules(const int32_t* hist_item, int P, const int32_t* first_pos, int n_item,
                                                 const int32_t* nbr_pos, const int32_t* nbr_count, int n_nbr,
                                                 const int32_t* cat_item, const int32_t* cat_cate, int N, const int32_t* excl, int E,
                                                 int include_seeds, const uint32_t* allow, int G, int32_t* cand_pos,
                                                 int32_t* cand_item, int32_t* cand_cate, int32_t* n_cand, int cap, int U,
                                                 rsx_stream_t stream) {
  return retrieve_launch(hist_item, P, first_pos, n_item, nbr_pos, nbr_count, n_nbr, cat_item, cat_cate, N, excl, E, include_seeds,
                         allow, G, cand_pos, cand_item, cand_cate, n_cand, cap, U, stream);
}
