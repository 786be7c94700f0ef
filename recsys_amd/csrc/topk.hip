// Top-k selection over rows of fp32 scores with a running list on the device (include/rsx.h rsx_topk_rows).  Generic over score
// rows: serving.Predictor.rank_candidates(top_k=k) runs it behind rsx_predict_din_rank, once per chunk of a long request.
//
// ORDER (the contract): higher score first; equal scores (-0.0 == +0.0) by lower index; every NaN below every number, NaNs by
// lower index among themselves -- np.lexsort((index, -score)).  Each entry becomes ONE 64-bit key whose unsigned order is that
// order:
//     bits 63..32  the order-preserving image of the score: sign set -> ~bits, else bits | 0x80000000; -0.0 takes +0.0's image
//                  and every NaN the image 0 (the smallest number, -inf, has image 0x007fffff)
//     bits 31..1   ~index (31 bits: indices stay below 2^31 - 1), so the lower index is the larger key
//     bit  0       "the score was -0.0": never decides anything (indices are unique) and lets the value be rebuilt from the key
// Keys are unique, so exactly `want` of them are >= the want-th largest and nothing depends on the order threads run in.
//
// ONE workgroup per row.  It (1) turns the row's running list (the first `filled` pairs of out_val / out_idx) and the n new
// scores (indices next_index ..) into keys in LDS -- every read of the old list happens before the first barrier, every write of
// the new list after the last, which is what makes the in-place update safe; (2) finds the want-th largest key, want =
// min(k, filled + n), by an MSB-first radix select, 8 bits a pass, over integer LDS histograms (order-independent), stopping as
// soon as the selected bin is taken whole; (3) compacts the keys >= that threshold (their order in the compacted list is
// arbitrary and does not matter); (4) gives every survivor its rank = the number of survivors with a larger key (unique keys:
// a permutation) and writes (value, index) at that rank.  The value is rebuilt from the key; a NaN -- whose payload the key does
// not hold -- is read again, from the scores or from the old list's copy in LDS.
//
// Histogram atomics: one plain LDS atomicAdd per matching key.  A form in which each wave first added the ballot count of its
// first lane's bin with one atomic was measured against this one (interleaved, 500 launches a round, n = 4 096, k = 100): 0.9 us
// slower on probabilities and on uniform scores (14.4 against 13.5 us with the state's zeroing), 18 us faster only when every
// score is equal (20.6 against 38.5 us: all 4 196 atomics of the first passes on one address).  The simpler loop stays.
#include "topk_device.h"         // the key image, the LDS plan and the workgroup's body, shared with topk_excl.hip

namespace {

__global__ __launch_bounds__(TK_T_BIG) void topk_rows_k(const TopkArgs p) {
  extern __shared__ unsigned long long tk_lds[];
  topk_rows_body<TK_PLAIN>(p, tk_lds);
}

}  // namespace

extern "C" int rsx_topk_rows_supported(int n, int k) { return topk_envelope(n, k) ? 1 : 0; }

extern "C" int rsx_topk_rows_threads(int n, int k) { return topk_envelope(n, k) ? (int)topk_threads(n, k) : 0; }

extern "C" int rsx_topk_rows(const float* scores, int ld, int U, int n, int k, float* out_val, int32_t* out_idx, int32_t* state,
                             rsx_stream_t stream) {
  if (!scores || !out_val || !out_idx || !state || U <= 0 || n <= 0 || k <= 0 || ld < n) return RSX_EINVAL;
  if (!topk_envelope(n, k)) return RSX_EUNSUPPORTED;
  TopkArgs p;
  p.scores = scores; p.out_val = out_val; p.out_idx = out_idx; p.state = state;
  p.ld = ld; p.n = n; p.k = k;
  const size_t lds = (size_t)topk_layout(&p);
  if (lds > (size_t)PR_MAX_LDS) return RSX_EUNSUPPORTED;
  return launch_big_lds<topk_rows_k>(p, (unsigned)U, topk_threads(n, k), lds, rsx_s(stream));
}
