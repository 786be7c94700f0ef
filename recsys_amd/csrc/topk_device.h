// What the top-k kernels share (topk.hip: rsx_topk_rows; topk_excl.hip: rsx_topk_rows_excl; topk_rules.hip:
// rsx_topk_rows_rules; topk_counted.hip: rsx_topk_rows_counted): the 64-bit key image of a (score, index) pair, the LDS plan, and the workgroup's body -- keys, MSB-first
// radix select, compaction, rank by counting.  topk.hip's head describes the method.  MODE TK_PLAIN is rsx_topk_rows; TK_EXCL
// adds the exclusion of new scores by id (topk_excl.hip's head); TK_RULES adds the category rules on top of that
// (topk_rules.hip's head).  Each addition is compiled in with `if constexpr`, so a kernel holds nothing of the modes above it.
// TK_COUNTED (topk_counted.hip: rsx_topk_rows_counted) is TK_PLAIN with a per-row count of valid new scores; it stands beside
// the three, not above them, and is compiled in the same way.  TK_CAPPED (topk_capped.hip: rsx_topk_lists_capped) is TK_COUNTED with
// TK_RULES' cap over per-row categories; the cap's rounds are one function (tk_cap) that both compile in.
#pragma once
#include "predict_device.h"      // launch_big_lds, PR_MAX_LDS

namespace {

constexpr int TK_KMAX = 1024;            // largest k
constexpr int TK_KEYS = 16384;           // largest n + k: 128 KB of keys
constexpr int TK_T_SMALL = 256, TK_T_BIG = 1024;
constexpr int TK_SMALL_KEYS = 1024;     // up to this many keys a workgroup of 256 threads, above it 1024
constexpr int TK_EMAX = 256;             // largest exclusion list of a row (EXCL)
constexpr int TK_MMAX = 16;              // largest per-category cap (RULES)
constexpr int TK_PLAIN = 0, TK_EXCL = 1, TK_RULES = 2, TK_COUNTED = -1, TK_CAPPED = -2;

struct TopkArgs {
  const float* scores;
  float* out_val;
  int32_t* out_idx;
  int32_t* state;
  int ld, n, k;
  int oSel, oOldV, oOldI, oHist, oMisc;  // LDS plan, in bytes from the start of the keys
};

struct TopkCountedArgs : TopkArgs {
  const int32_t* n_valid;                // [U]: new score j of row u is left out when j >= n_valid[u]
};

struct TopkCappedArgs : TopkCountedArgs {
  const int32_t* cate;                   // [U, ld_cate]: row u's categories by absolute index, cate[u * ld_cate + a]
  int ld_cate, G, m;                     // columns of a cate row, categories, cap (0: none)
  int oThr, oCat;                        // LDS (m > 0): as TopkRulesArgs'
};

struct TopkExclArgs : TopkArgs {
  const int32_t* cand_id;                // [n], shared by the rows
  const int32_t* excl;                   // [U, E]
  int E;
  int oExcl;                             // LDS: the row's exclusion ids, sorted [E]
};

struct TopkRulesArgs : TopkExclArgs {
  const int32_t* cate;                   // [next_index + n]: the category of every entry fed so far, by absolute index
  const uint32_t* allow;                 // [U, W] bitmap of the allowed categories, or null (all allowed)
  int G, W, m;                           // categories, words of a bitmap row, cap (0: none)
  int oThr, oCat;                        // LDS (m > 0): two [G] arrays of 64-bit thresholds; the keys' categories, 16 bits each
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

// The exclusion list of a row (EXCL; rank_count.hip uses the same two steps).  tk_excl_sort: the E ids of `ex` rank-sorted into
// LDS at exs, with `raw` (LDS, E words) as the unsorted copy; every thread of the workgroup calls it, and a barrier must follow
// before exs is read.  tk_excluded: whether `id` is a positive entry of the sorted list -- a binary search, <= 8 LDS reads.
__device__ __forceinline__ void tk_excl_sort(const int32_t* ex, const int E, int* raw, int* exs, const int tid, const int NT) {
  for (int t = tid; t < E; t += NT) {
    const int v = ex[t];
    raw[t] = v > 0 ? v : 0;
  }
  __syncthreads();
  for (int t = tid; t < E; t += NT) {
    const int v = raw[t];
    int rank = 0;
    for (int j = 0; j < E; ++j) {
      const int o = raw[j];
      rank += (o < v || (o == v && j < t)) ? 1 : 0;
    }
    exs[rank] = v;
  }
}

__device__ __forceinline__ bool tk_excluded(const int* exs, const int E, const int id) {
  int lo = 0, hi = E;                                                // lower bound of id in exs
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (exs[mid] < id) lo = mid + 1; else hi = mid;
  }
  return id > 0 && lo < E && exs[lo] == id;
}

// The cap (RULES, CAPPED).  thr[g] = the m-th largest key of category g among the T keys (0 when g holds fewer than m live keys),
// found in m rounds: in round r every live key below its category's threshold of round r - 1 (round 0: every live key) is max-ed
// into the category's slot.  Keys are unique and max is commutative, so the thresholds do not depend on the order threads run
// in.  (The plain read before the atomic only spares the atomic where it could change nothing: a slot only grows inside a
// round.)  A key below its threshold has m category mates above it and takes key 0 -- an entry of the running list included.
// kcat: the keys' categories, each inside [0, G) wherever the key is not 0; thr: two [G] arrays; left: an LDS counter.  Every
// thread of the workgroup calls it, after writing its keys and categories and before any barrier; -> the number of keys left.
__device__ __forceinline__ int tk_cap(unsigned long long* keys, const unsigned short* kcat, unsigned long long* thr, const int G,
                                      const int m, const int T, unsigned* left_at, const int tid, const int NT) {
  unsigned long long* cur = thr;
  unsigned long long* prev = cur + G;
  for (int g = tid; g < 2 * G; g += NT) cur[g] = 0ull;
  if (tid == 0) *left_at = 0u;
  __syncthreads();
  for (int r = 0; r < m; ++r) {
    if (r >= 2) {                                                    // this round's slots held the thresholds of round r - 2
      for (int g = tid; g < G; g += NT) cur[g] = 0ull;
      __syncthreads();
    }
    for (int i = tid; i < T; i += NT) {
      const unsigned long long key = keys[i];
      if (key == 0ull) continue;
      const int c = kcat[i];
      if (r > 0 && key >= prev[c]) continue;
      if (key > __hip_atomic_load(&cur[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(&cur[c], key);
    }
    __syncthreads();
    unsigned long long* t = cur; cur = prev; prev = t;
  }
  unsigned left = 0u;
  for (int i = tid; i < T; i += NT) {
    const unsigned long long key = keys[i];
    if (key == 0ull) continue;
    if (key < prev[kcat[i]]) keys[i] = 0ull; else ++left;
  }
  if (left) atomicAdd(left_at, left);
  __syncthreads();
  return (int)*left_at;
}

template <int MODE, class Args>
__device__ __forceinline__ void topk_rows_body(const Args& p, unsigned long long* tk_lds) {
  constexpr bool EXCL = MODE >= TK_EXCL, RULES = MODE == TK_RULES, CAPPED = MODE == TK_CAPPED,
                 COUNTED = MODE == TK_COUNTED || CAPPED;
  unsigned long long* keys = tk_lds;
  char* base = reinterpret_cast<char*>(tk_lds);
  unsigned long long* sel = reinterpret_cast<unsigned long long*>(base + p.oSel);
  float* oldv = reinterpret_cast<float*>(base + p.oOldV);
  int* oldi = reinterpret_cast<int*>(base + p.oOldI);
  unsigned* hist = reinterpret_cast<unsigned*>(base + p.oHist);
  unsigned* misc = reinterpret_cast<unsigned*>(base + p.oMisc);      // 0: bin, 1: rank inside the bin, 2: the bin's count, 3: compaction cursor (EXCL: 4: new scores kept; RULES, CAPPED: 5: keys left under the cap)

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

  // (1) keys of the running list and of the new scores
  for (int i = tid; i < filled; i += NT) {
    const float v = ov[i];
    const int ix = oi[i];
    oldv[i] = v;
    oldi[i] = ix;
    keys[i] = tk_key(v, ix);
  }
  if constexpr (RULES) {
    // Under a cap the running list's entries need their category again: from `cate` by their absolute index, into the cache.
    // An index that is not one fed before, or a category outside [0, G), takes key 0 and indexes nothing.
    if (p.m > 0) {
      unsigned short* kcat = reinterpret_cast<unsigned short*>(base + p.oCat);
      for (int i = tid; i < filled; i += NT) {
        const int ix = oi[i];
        const int c = (ix >= 0 && ix < next0) ? p.cate[ix] : -1;
        const bool ok = c >= 0 && c < p.G;
        kcat[i] = (unsigned short)(ok ? c : 0);
        if (!ok) keys[i] = 0ull;
      }
    }
  }
  if constexpr (CAPPED) {
    // The same with the row's own categories, cate[row, index]; an index at or beyond ld_cate is not one the caller gave.
    if (p.m > 0) {
      unsigned short* kcat = reinterpret_cast<unsigned short*>(base + p.oCat);
      const int32_t* cg = p.cate + row * (size_t)p.ld_cate;
      for (int i = tid; i < filled; i += NT) {
        const int ix = oi[i];
        const int c = (ix >= 0 && ix < next0 && ix < p.ld_cate) ? cg[ix] : -1;
        const bool ok = c >= 0 && c < p.G;
        kcat[i] = (unsigned short)(ok ? c : 0);
        if (!ok) keys[i] = 0ull;
      }
    }
  }
  if (tid == 0) misc[3] = 0u;
  int want;
  if constexpr (EXCL) {
    // The row's exclusion ids, sorted into LDS: entries <= 0 (padding) become 0 and sort first.  The unsorted copy borrows the
    // histogram's 256 words (E <= 256; the select zeroes them before every pass).  Rank = the number of entries that sort
    // before this one, ties by position: a permutation, whatever order the threads run in.
    const int E = p.E;
    int* exs = reinterpret_cast<int*>(base + p.oExcl);
    if (tid == 0) misc[4] = 0u;
    if (E > 0) tk_excl_sort(p.excl + row * (size_t)E, E, reinterpret_cast<int*>(hist), exs, tid, NT);
    __syncthreads();
    // An excluded score takes key 0: below every real key (tk_key gives 0 only for a NaN at index 2^31 - 1, which the contract
    // rules out), so it is never among the `want` largest when want counts the kept keys only.
    unsigned kept = 0u;
    for (int j = tid; j < n; j += NT) {
      bool out = E > 0 && tk_excluded(exs, E, p.cand_id[j]);
      if constexpr (RULES) {
        // A new score also leaves when its category is outside [0, G) or its bit of the row's bitmap is clear.
        if (p.allow || p.m > 0) {
          const int c = p.cate[(size_t)next0 + j];
          const bool ok = c >= 0 && c < p.G;
          if (!ok) out = true;
          else if (p.allow) out = out || !((p.allow[row * (size_t)p.W + (c >> 5)] >> (c & 31)) & 1u);
          if (p.m > 0) reinterpret_cast<unsigned short*>(base + p.oCat)[filled + j] = (unsigned short)(ok ? c : 0);
        }
      }
      keys[filled + j] = out ? 0ull : tk_key(sc[j], next0 + j);
      kept += out ? 0u : 1u;
    }
    if (kept) atomicAdd(&misc[4], kept);                             // (integer: the sum does not depend on the order)
    __syncthreads();
    const int Te = filled + (int)misc[4];
    want = Te < k ? Te : k;
    if constexpr (RULES) {
      if (p.m > 0) {
        // The cap (tk_cap): a key with m category mates above it takes key 0; want counts what is left.
        const int Tl = tk_cap(keys, reinterpret_cast<const unsigned short*>(base + p.oCat),
                              reinterpret_cast<unsigned long long*>(base + p.oThr), p.G, p.m, T, &misc[5], tid, NT);
        want = Tl < k ? Tl : k;
      }
    }
  } else if constexpr (COUNTED) {
    // The new scores at and beyond the row's count take key 0, as an excluded score does; they are never read.
    int nv = p.n_valid[row];
    nv = nv < 0 ? 0 : (nv > n ? n : nv);
    want = filled + nv < k ? filled + nv : k;
    if constexpr (CAPPED) {
      if (p.m > 0) {
        // A live new score needs a category inside [0, G) -- else key 0 -- and caches it; behind the count neither the score
        // nor the category is read.  Then the cap over the union; want counts what is left.
        unsigned short* kcat = reinterpret_cast<unsigned short*>(base + p.oCat);
        const int32_t* cg = p.cate + row * (size_t)p.ld_cate;
        for (int j = tid; j < n; j += NT) {
          int c = -1;
          if (j < nv && (long long)next0 + j < p.ld_cate) c = cg[next0 + j];
          const bool ok = c >= 0 && c < p.G;
          keys[filled + j] = ok ? tk_key(sc[j], next0 + j) : 0ull;
          kcat[filled + j] = (unsigned short)(ok ? c : 0);
        }
        const int Tl = tk_cap(keys, kcat, reinterpret_cast<unsigned long long*>(base + p.oThr), p.G, p.m, T, &misc[5], tid, NT);
        want = Tl < k ? Tl : k;
      } else {
        for (int j = tid; j < n; j += NT) keys[filled + j] = j < nv ? tk_key(sc[j], next0 + j) : 0ull;
        __syncthreads();
      }
    } else {
      for (int j = tid; j < n; j += NT) keys[filled + j] = j < nv ? tk_key(sc[j], next0 + j) : 0ull;
      __syncthreads();
    }
  } else {
    want = T < k ? T : k;
    for (int j = tid; j < n; j += NT) keys[filled + j] = tk_key(sc[j], next0 + j);
    __syncthreads();
  }

  // The select runs when the keys outnumber the survivors.  Plain: T > k, and then want == k.  EXCL: also when excluded keys
  // (zeros) sit among no more than k kept ones (filled + kept < k < filled + n included) -- the want-th largest key is a real
  // one, every zero is smaller, and a bin that holds a zero is never "taken whole", so `key >= prefix` admits no zero.
  // RULES: the same argument, wherever the zeros sit -- under a cap entries of the running list become zeros too.
  // COUNTED: EXCL's argument with the zeros behind the row's count.  CAPPED: RULES' argument.
  const int nsel = (EXCL || COUNTED) ? want : k;
  const bool select = (EXCL || COUNTED) ? (T > want && want > 0) : (T > k);
  const unsigned long long* src = keys;                            // the survivors: everything when the union is no longer than k
  if (select) {
    // (2) radix select of the nsel-th largest key
    unsigned long long prefix = 0ull, mask = 0ull;
    unsigned r = (unsigned)nsel;                                   // the key wanted is the r-th largest of those matching the prefix
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
    // (3) the keys >= prefix are exactly nsel
    for (int i = tid; i < T; i += NT) {
      const unsigned long long key = keys[i];
      if (key >= prefix) {
        const unsigned at = atomicAdd(&misc[3], 1u);
        if (at < (unsigned)nsel) sel[at] = key;
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
inline unsigned topk_threads(int n, int k) { return n + k <= TK_SMALL_KEYS ? TK_T_SMALL : TK_T_BIG; }

inline int topk_layout(TopkArgs* p) {
  int o = 8 * (p->n + p->k);
  p->oSel = o; o += 8 * p->k;
  p->oOldV = o; o += 4 * p->k;
  p->oOldI = o; o += 4 * p->k;
  p->oHist = o; o += 4 * 256;
  p->oMisc = o; o += 16;
  return o;
}

inline bool topk_excl_envelope(int n, int k, int E) { return topk_envelope(n, k) && E >= 0 && E <= TK_EMAX; }

inline int topk_excl_layout(TopkExclArgs* p) {
  int o = topk_layout(p);
  o += 16;                               // misc[4 .. 7]: the count of kept scores (RULES: and of the keys left under the cap)
  p->oExcl = o; o += 4 * TK_EMAX;
  return o;
}

// RULES: without a cap (m == 0) the plan is rsx_topk_rows_excl's; a cap adds the two threshold arrays and the category cache.
// -1: not a plan (m outside [0, 16], a cap without categories, or more than the LDS can ever hold).
inline long long topk_rules_layout(TopkRulesArgs* p) {
  long long o = topk_excl_layout(p);
  p->oThr = p->oCat = 0;
  if (p->m < 0 || p->m > TK_MMAX) return -1;
  if (p->m > 0) {
    if (p->G <= 0 || p->G > 65535) return -1;                  // (16 bits of category cache a key)
    p->oThr = (int)o; o += 16ll * p->G;
    p->oCat = (int)o; o += 2ll * (p->n + p->k);              // (last: nothing behind it needs an alignment)
  }
  return o;
}

// CAPPED: without a cap (m == 0) the plan is rsx_topk_rows_counted's; a cap adds 16 bytes behind misc (the counter of the keys
// left), the two threshold arrays and the category cache.  -1: not a plan (m outside [0, 16], G outside [1, 65 535] under a cap).
inline long long topk_capped_layout(TopkCappedArgs* p) {
  long long o = topk_layout(p);
  p->oThr = p->oCat = 0;
  if (p->m < 0 || p->m > TK_MMAX) return -1;
  if (p->m > 0) {
    if (p->G <= 0 || p->G > 65535) return -1;
    o += 16;
    p->oThr = (int)o; o += 16ll * p->G;
    p->oCat = (int)o; o += 2ll * (p->n + p->k);
  }
  return o;
}

}  // namespace
