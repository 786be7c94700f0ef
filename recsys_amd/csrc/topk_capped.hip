// rsx_topk_rows_counted with a per-category cap over per-row categories (include/rsx.h rsx_topk_lists_capped): every entry of
// row u has a category, cate[u * ld_cate + absolute index], and the row keeps at most m entries of one category.
// serving.Predictor.recommend_two_stage runs it in rsx_topk_rows_counted's place when a request names max_per_category, with the
// candidate categories rsx_din_retrieve_candidates wrote into the rank launch's candidate buffer as `cate`.
//
// The kernel is topk_counted.hip's (topk_device.h, MODE TK_CAPPED) with topk_rules.hip's cap:
//   - a LIVE new score (j < n_valid[u]) whose category is outside [0, G) takes key 0, as a score behind the count does; behind
//     the count neither the score nor the category is read;
//   - the cap works on the keys of the union, the running list's included (tk_cap: per category the m-th largest key by m rounds
//     of one 64-bit LDS atomicMax per live key, two [G] arrays, ping-pong; a key below its category's threshold takes key 0).
//     Keys are unique and max is commutative: nothing depends on the order threads run in.  want = min(k, keys left).
// The running list of k entries is exact for the reason topk_rules.hip's head gives: adding entries never lowers the number of
// category mates above an entry, so capped_topk(seen + chunk) == capped_topk(capped_topk(seen) + chunk).
//
// LDS with a cap = rsx_topk_rows_counted's plan + 16 + 16 G + 2 (n + k) bytes = 10 (n + k) + 16 k + 1 056 + 16 G: for G = 802 and
// k = 1 024 that is 10 (n + k) + 30 272 <= 163 840, so n + k <= 13 356.  A candidate list of 3 328 columns with k = 1 024 takes
// 73 792 bytes: one workgroup of 1 024 threads per compute unit, as the whole family above 1 024 keys.  Without a cap (m == 0)
// the plan is rsx_topk_rows_counted's and so is every instruction that runs: the same outputs and state, bit for bit.
// All keys of one category and m = 1 is the family's slow case (topk.hip's head): every atomic of a round on one address.
#include "topk_device.h"

namespace {

__global__ __launch_bounds__(TK_T_BIG) void topk_lists_capped_k(const TopkCappedArgs p) {
  extern __shared__ unsigned long long tk_lds[];
  topk_rows_body<TK_CAPPED>(p, tk_lds);
}

// -> the LDS bytes of the plan, or -1 outside the envelope
inline long long topk_capped_plan(TopkCappedArgs* p) {
  if (!topk_envelope(p->n, p->k)) return -1;
  const long long o = topk_capped_layout(p);
  return (o < 0 || o > (long long)PR_MAX_LDS) ? -1 : o;
}

}  // namespace

extern "C" int rsx_topk_lists_capped_supported(int n, int k, int G, int m) {
  TopkCappedArgs p{};
  p.n = n; p.k = k; p.G = G; p.m = m;
  if (G < 0) return 0;
  return topk_capped_plan(&p) >= 0 ? 1 : 0;
}

extern "C" int rsx_topk_lists_capped(const float* scores, int ld, const int32_t* n_valid, const int32_t* cate, int ld_cate, int G,
                                     int m, int U, int n, int k, float* out_val, int32_t* out_idx, int32_t* state,
                                     rsx_stream_t stream) {
  if (!scores || !n_valid || !out_val || !out_idx || !state || U <= 0 || n <= 0 || k <= 0 || ld < n || m < 0) return RSX_EINVAL;
  if (m > 0 && (!cate || G <= 0 || ld_cate < n)) return RSX_EINVAL;
  TopkCappedArgs p{};
  p.scores = scores; p.out_val = out_val; p.out_idx = out_idx; p.state = state;
  p.ld = ld; p.n = n; p.k = k;
  p.n_valid = n_valid;
  p.cate = cate; p.ld_cate = ld_cate; p.G = m > 0 ? G : 0; p.m = m;
  const long long o = topk_capped_plan(&p);
  if (o < 0) return RSX_EUNSUPPORTED;
  return launch_big_lds<topk_lists_capped_k>(p, (unsigned)U, topk_threads(n, k), (size_t)o, rsx_s(stream));
}
