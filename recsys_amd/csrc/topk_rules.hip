// rsx_topk_rows_excl with category rules (include/rsx.h rsx_topk_rows_rules): every entry has a category, cate[absolute index],
// and a row may (a) allow only the categories whose bit is set in its bitmap allow[u, :W] and (b) keep at most m entries of one
// category.  serving.Predictor.recommend runs it in rsx_topk_rows_excl's place when a request names a rule, with the resident
// catalogue's categories as `cate`.
//
// The kernel is topk_excl.hip's (topk_device.h, MODE TK_RULES) with two additions:
//   - (a) is one more reason for a NEW score to take key 0, beside the exclusion by id: a category outside [0, G) or a clear
//     bit.  The running list is not looked at: what it holds passed the same bitmap when it entered.
//   - (b) works on the keys of the union, the running list's included.  The capped answer is the top k of the entries that have
//     fewer than m category mates above them, so the kernel finds per category the m-th largest key -- m rounds of one 64-bit
//     LDS atomicMax per live key into thr[category], round r admitting only keys below round r - 1's threshold (two [G] arrays,
//     ping-pong) -- and gives every key below its category's threshold key 0.  Keys are unique and max is commutative: nothing
//     depends on the order threads run in.  want = min(k, keys left); select, compaction and ranks are unchanged, since the
//     select's argument never cared where the zeros sit.
// Why the running list of k entries is enough: adding entries never lowers the number of category mates above an entry, so an
// entry that left the capped top k of what was fed so far never returns, and every entry the list keeps has all its
// higher-ranked category mates in the list too: capped_topk(seen + chunk) == capped_topk(capped_topk(seen) + chunk).
//
// The keys' categories are cached in LDS, 16 bits a key, when m > 0: the rounds and the drop read them m + 1 times, and the
// running list's would otherwise be m + 1 gathers from global memory.  LDS with a cap = rsx_topk_rows_excl's plan + 16 G +
// 2 (n + k) bytes: for G = 802, k = 1 024 that is 10 (n + k) + 31 296 <= 163 840, so n + k <= 13 254 (rsx_topk_rows_excl:
// 16 384).  Without a cap (m == 0) the plan is rsx_topk_rows_excl's, and with allow == NULL as well so is every instruction
// that runs: the same outputs and state, bit for bit.
// All keys of one category and m = 1 is the family's slow case (topk.hip's head): every atomic of a round on one address.  The
// plain read before the atomic skips those that cannot raise the slot; correctness does not depend on it.
#include "topk_device.h"

namespace {

__global__ __launch_bounds__(TK_T_BIG) void topk_rows_rules_k(const TopkRulesArgs p) {
  extern __shared__ unsigned long long tk_lds[];
  topk_rows_body<TK_RULES>(p, tk_lds);
}

// -> the LDS bytes of the plan, or -1 outside the envelope
inline long long topk_rules_plan(TopkRulesArgs* p, int E) {
  if (!topk_excl_envelope(p->n, p->k, E)) return -1;
  const long long o = topk_rules_layout(p);
  return (o < 0 || o > (long long)PR_MAX_LDS) ? -1 : o;
}

}  // namespace

extern "C" int rsx_topk_rows_rules_supported(int n, int k, int E, int G, int m) {
  TopkRulesArgs p{};
  p.n = n; p.k = k; p.G = G; p.m = m;
  if (G < 0) return 0;
  return topk_rules_plan(&p, E) >= 0 ? 1 : 0;
}

extern "C" int rsx_topk_rows_rules(const float* scores, int ld, const int32_t* cand_id, const int32_t* excl, int E,
                                   const int32_t* cate, int G, const uint32_t* allow, int m, int U, int n, int k, float* out_val,
                                   int32_t* out_idx, int32_t* state, rsx_stream_t stream) {
  if (!scores || !cand_id || !out_val || !out_idx || !state || U <= 0 || n <= 0 || k <= 0 || ld < n || E < 0 || m < 0) return RSX_EINVAL;
  if (E > 0 && !excl) return RSX_EINVAL;
  const bool rules = allow != nullptr || m > 0;
  if (rules && (!cate || G <= 0)) return RSX_EINVAL;
  TopkRulesArgs p{};
  p.scores = scores; p.out_val = out_val; p.out_idx = out_idx; p.state = state;
  p.ld = ld; p.n = n; p.k = k;
  p.cand_id = cand_id; p.excl = excl; p.E = E;
  p.cate = cate; p.allow = allow; p.G = rules ? G : 0; p.W = p.G / 32 + (p.G % 32 ? 1 : 0); p.m = m;
  const long long o = topk_rules_plan(&p, E);
  if (o < 0) return RSX_EUNSUPPORTED;
  return launch_big_lds<topk_rows_rules_k>(p, (unsigned)U, topk_threads(n, k), (size_t)o, rsx_s(stream));
}
