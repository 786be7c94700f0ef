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
#include "predict_device.h"      // launch_big_lds

namespace {

constexpr int TK_KMAX = 1024;            // largest k
constexpr int TK_KEYS = 16384;           // largest n + k: 128 KB of keys
constexpr int TK_T_SMALL = 256, TK_T_BIG = 1024;
constexpr int TK_SMALL_KEYS = 1024;     // up to this many keys a workgroup of 256 threads, above it 1024

struct TopkArgs {
  const float* scores;
  float* out_val;
  int32_t* out_idx;
  int32_t* state;
  int ld, n, k;
  int oSel, oOldV, oOldI, oHist, oMisc;  // LDS plan, in bytes from the start of the keys
};

__device__ __forceinline__ unsigned long long tk_key(const float v, const int idx) {
  unsigned u = __float_as_uint(v);
  const bool negzero = u == 0x80000000u;
  if (negzero) u = 0u;
  unsigned img = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  if ((u & 0x7fffffffu) > 0x7f800000u) img = 0u;
  const unsigned lo = ((~(unsigned)idx & 0x7fffffffu) << 1) | (negzero ? 1u : 0u);
  return ((unsigned long long)img << 32) | lo;
}

__device__ __forceinline__ int tk_index(const unsigned long long key) { return (int)(~((unsigned)key >> 1) & 0x7fffffffu); }

__global__ __launch_bounds__(TK_T_BIG) void topk_rows_k(const TopkArgs p) {
  extern __shared__ unsigned long long tk_lds[];
  unsigned long long* keys = tk_lds;
  char* base = reinterpret_cast<char*>(tk_lds);
  unsigned long long* sel = reinterpret_cast<unsigned long long*>(base + p.oSel);
  float* oldv = reinterpret_cast<float*>(base + p.oOldV);
  int* oldi = reinterpret_cast<int*>(base + p.oOldI);
  unsigned* hist = reinterpret_cast<unsigned*>(base + p.oHist);
  unsigned* misc = reinterpret_cast<unsigned*>(base + p.oMisc);      // 0: bin, 1: rank inside the bin, 2: the bin's count, 3: compaction cursor

  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
  const int n = p.n, k = p.k;
  const size_t row = blockIdx.x;
  const float* sc = p.scores + row * (size_t)p.ld;
  float* ov = p.out_val + row * (size_t)k;
  int32_t* oi = p.out_idx + row * (size_t)k;
  int32_t* st = p.state + row * 2;

  int filled = st[0];
  const int next0 = st[1];
  filled = filled < 0 ? 0 : (filled > k ? k : filled);             // a state nobody zeroed must not index out of the list
  const int T = filled + n;
  const int want = T < k ? T : k;

  // (1) keys of the running list and of the new scores
  for (int i = tid; i < filled; i += NT) {
    const float v = ov[i];
    const int ix = oi[i];
    oldv[i] = v;
    oldi[i] = ix;
    keys[i] = tk_key(v, ix);
  }
  for (int j = tid; j < n; j += NT) keys[filled + j] = tk_key(sc[j], next0 + j);
  if (tid == 0) misc[3] = 0u;
  __syncthreads();

  const unsigned long long* src = keys;                            // the survivors: everything when the union is no longer than k
  if (T > k) {
    // (2) radix select of the k-th largest key
    unsigned long long prefix = 0ull, mask = 0ull;
    unsigned r = (unsigned)k;                                      // the key wanted is the r-th largest of those matching the prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
      for (int b = tid; b < 256; b += NT) hist[b] = 0u;
      __syncthreads();
      for (int i = tid; i < T; i += NT) {
        const unsigned long long key = keys[i];
        if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid < 64) {                                              // lane l owns bins 4 l .. 4 l + 3; higher bins are larger keys
        const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        const unsigned s = c0 + c1 + c2 + c3;
        unsigned suf = s;                                          // -> sum over lanes >= this one
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned t = (unsigned)__shfl_down((int)suf, d);
          if (lane + d < 64) suf += t;
        }
        unsigned a = suf - s;                                      // keys in the bins of higher lanes
        if (a < r && r <= suf) {                                   // exactly one lane: 1 <= r <= the number of matching keys
          unsigned bin, cnt;
          if (r <= a + c3) { bin = 3u; cnt = c3; }
          else {
            a += c3;
            if (r <= a + c2) { bin = 2u; cnt = c2; }
            else {
              a += c2;
              if (r <= a + c1) { bin = 1u; cnt = c1; }
              else { a += c1; bin = 0u; cnt = c0; }
            }
          }
          misc[0] = 4u * lane + bin;
          misc[1] = r - a;
          misc[2] = cnt;
        }
      }
      __syncthreads();
      prefix |= (unsigned long long)misc[0] << shift;
      mask |= 255ull << shift;
      r = misc[1];
      if (misc[2] == r) break;                                     // the bin is taken whole: every key >= prefix is in
    }
    // (3) the keys >= prefix are exactly k
    for (int i = tid; i < T; i += NT) {
      const unsigned long long key = keys[i];
      if (key >= prefix) {
        const unsigned at = atomicAdd(&misc[3], 1u);
        if (at < (unsigned)k) sel[at] = key;
      }
    }
    __syncthreads();
    src = sel;
  }

  // (4) rank = the number of survivors with a larger key; write (value, index) there
  for (int w = tid; w < want; w += NT) {
    const unsigned long long key = src[w];
    int rank = 0;
    for (int j = 0; j < want; ++j) rank += src[j] > key ? 1 : 0;
    const unsigned img = (unsigned)(key >> 32);
    const int idx = tk_index(key);
    float v;
    if (img != 0u) {
      unsigned u = (img & 0x80000000u) ? (img ^ 0x80000000u) : ~img;
      if (key & 1ull) u = 0x80000000u;
      v = __uint_as_float(u);
    } else if (idx >= next0 && idx - next0 < n) {                  // a NaN of this call: its bits are in the scores
      v = sc[idx - next0];
    } else {                                                       // a NaN of the running list: its bits are in the LDS copy
      v = __uint_as_float(0x7fc00000u);
      for (int j = 0; j < filled; ++j)
        if (oldi[j] == idx) v = oldv[j];
    }
    ov[rank] = v;
    oi[rank] = idx;
  }
  if (tid == 0) {
    st[0] = want;
    st[1] = next0 + n;
  }
}

inline bool topk_envelope(int n, int k) { return n >= 1 && k >= 1 && k <= TK_KMAX && (long long)n + k <= TK_KEYS; }

size_t topk_layout(TopkArgs* p) {
  int o = 8 * (p->n + p->k);
  p->oSel = o; o += 8 * p->k;
  p->oOldV = o; o += 4 * p->k;
  p->oOldI = o; o += 4 * p->k;
  p->oHist = o; o += 4 * 256;
  p->oMisc = o; o += 16;
  return (size_t)o;
}

}  // namespace

extern "C" int rsx_topk_rows_supported(int n, int k) { return topk_envelope(n, k) ? 1 : 0; }

extern "C" int rsx_topk_rows(const float* scores, int ld, int U, int n, int k, float* out_val, int32_t* out_idx, int32_t* state,
                             rsx_stream_t stream) {
  if (!scores || !out_val || !out_idx || !state || U <= 0 || n <= 0 || k <= 0 || ld < n) return RSX_EINVAL;
  if (!topk_envelope(n, k)) return RSX_EUNSUPPORTED;
  TopkArgs p;
  p.scores = scores; p.out_val = out_val; p.out_idx = out_idx; p.state = state;
  p.ld = ld; p.n = n; p.k = k;
  const size_t lds = topk_layout(&p);
  if (lds > (size_t)PR_MAX_LDS) return RSX_EUNSUPPORTED;
  const unsigned threads = n + k <= TK_SMALL_KEYS ? TK_T_SMALL : TK_T_BIG;
  return launch_big_lds<topk_rows_k>(p, (unsigned)U, threads, lds, rsx_s(stream));
}
