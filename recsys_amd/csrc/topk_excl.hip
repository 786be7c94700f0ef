// rsx_topk_rows with a filter on the NEW scores (include/rsx.h rsx_topk_rows_excl): score j of row u is left out of the union
// when cand_id[j] -- one id per column, shared by the rows -- equals a positive entry of the row's exclusion list excl[u, :E].
// serving.Predictor.recommend runs it behind rsx_predict_din_rank_shared over every chunk of the resident catalogue, with the
// user's history (and the caller's further ids) as the list: seen items never enter the running list.
//
// The kernel is topk.hip's (topk_device.h: key image, radix select, rank by counting) with three additions:
//   - the row's E ids go to LDS once, padding (<= 0) as 0, and are rank-sorted there (E <= 256: E compares per entry);
//   - every new score looks its id up by binary search (<= 8 LDS reads) -- membership depends on the ids alone, not on the
//     order threads run in; an excluded score becomes key 0, below every real key, and the kept ones are counted (an integer
//     LDS atomic per thread);
//   - want = min(k, filled + kept), and the select also runs when zeros sit among no more than k kept keys.
// The running list is never filtered; next_index advances by n, so indices stay positions on the column axis.  With E = 0 or
// only padding no key is 0 and every step is rsx_topk_rows': the same outputs and state, bit for bit.
// LDS at the envelope's edge (n + k = 16 384, k = 1 024): rsx_topk_rows' 148 496 bytes + 16 + 1 024 = 149 536 of 163 840.
#include "topk_device.h"

namespace {

__global__ __launch_bounds__(TK_T_BIG) void topk_rows_excl_k(const TopkExclArgs p) {
  extern __shared__ unsigned long long tk_lds[];
  topk_rows_body<TK_EXCL>(p, tk_lds);
}

}  // namespace

extern "C" int rsx_topk_rows_excl_supported(int n, int k, int E) { return topk_excl_envelope(n, k, E) ? 1 : 0; }

extern "C" int rsx_topk_rows_excl(const float* scores, int ld, const int32_t* cand_id, const int32_t* excl, int E, int U, int n,
                                  int k, float* out_val, int32_t* out_idx, int32_t* state, rsx_stream_t stream) {
  if (!scores || !cand_id || !out_val || !out_idx || !state || U <= 0 || n <= 0 || k <= 0 || ld < n || E < 0) return RSX_EINVAL;
  if (E > 0 && !excl) return RSX_EINVAL;
  if (!topk_excl_envelope(n, k, E)) return RSX_EUNSUPPORTED;
  TopkExclArgs p;
  p.scores = scores; p.out_val = out_val; p.out_idx = out_idx; p.state = state;
  p.ld = ld; p.n = n; p.k = k;
  p.cand_id = cand_id; p.excl = excl; p.E = E;
  const int o = topk_excl_layout(&p);
  if ((size_t)o > (size_t)PR_MAX_LDS) return RSX_EUNSUPPORTED;
  return launch_big_lds<topk_rows_excl_k>(p, (unsigned)U, topk_threads(n, k), (size_t)o, rsx_s(stream));
}
