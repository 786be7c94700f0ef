// rsx_topk_rows with a per-row count of valid new scores (include/rsx.h rsx_topk_rows_counted): score j of row u is left out of
// the union when j >= n_valid[u].  serving.Predictor.recommend_two_stage runs it behind rsx_predict_din_rank over the users'
// candidate lists [U, cap]: a list is padded to cap with (item 0, category 0), whose probability is a real number and must not
// enter the running list.
//
// The kernel is topk.hip's (topk_device.h: key image, radix select, rank by counting) with two additions:
//   - a new score at or beyond the row's count becomes key 0, below every real key, and is never read;
//   - want = min(k, filled + the count), and the select also runs when zeros sit among no more than k kept keys -- the argument
//     of topk_excl.hip.  The count needs no counter: it is the row's own word, clamped into [0, n].
// The running list is never filtered; next_index advances by n.  With n_valid[u] >= n no key is 0 and every step is
// rsx_topk_rows': the same outputs and state, bit for bit.  The LDS plan and the thread count are rsx_topk_rows'.
#include "topk_device.h"

namespace {

__global__ __launch_bounds__(TK_T_BIG) void topk_rows_counted_k(const TopkCountedArgs p) {
  extern __shared__ unsigned long long tk_lds[];
  topk_rows_body<TK_COUNTED>(p, tk_lds);
}

}  // namespace

extern "C" int rsx_topk_rows_counted(const float* scores, int ld, const int32_t* n_valid, int U, int n, int k, float* out_val,
                                     int32_t* out_idx, int32_t* state, rsx_stream_t stream) {
  if (!scores || !n_valid || !out_val || !out_idx || !state || U <= 0 || n <= 0 || k <= 0 || ld < n) return RSX_EINVAL;
  if (!topk_envelope(n, k)) return RSX_EUNSUPPORTED;
  TopkCountedArgs p;
  p.scores = scores; p.out_val = out_val; p.out_idx = out_idx; p.state = state;
  p.ld = ld; p.n = n; p.k = k;
  p.n_valid = n_valid;
  const size_t lds = (size_t)topk_layout(&p);
  if (lds > (size_t)PR_MAX_LDS) return RSX_EUNSUPPORTED;
  return launch_big_lds<topk_rows_counted_k>(p, (unsigned)U, topk_threads(n, k), lds, rsx_s(stream));
}
