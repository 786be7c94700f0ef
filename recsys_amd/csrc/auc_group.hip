// GAUC on gfx950 (include/rsx.h rsx_auc_group_*): the exact, tie-aware ROC AUC of csrc/auc_exact.hip made segmented -- one AUC per
// group (a user, an item category, ...), which the host weights by the group's impressions as the DIN paper does.  Opt-in, beside
// the 200-threshold tf.metrics.auc of csrc/metrics.hip and beside AUC_exact; it changes neither.
//
// THE CONTRACT, in integers.  An example is (group g, fp32 p, label y).  k32 is csrc/auc_exact.hip's 32-bit key exactly:
// (bits(p) << 1) | positive for a valid p, by the example rule of csrc/eval_device.h, the padding key otherwise.  The example is
// valid when k32 is not the padding key and 0 <= g < 2^group_bits (group_bits in 1..31).  A valid example is ONE 64-bit key
//     (uint64(g) << 32) | k32            unsigned key order = (group, score, label) order
// and an invalid one the padding key 0xFFFFFFFFFFFFFFFF, which sorts to the end, takes no part and is counted.  Over the sorted
// valid keys let
//     c[i]  the negatives in front of position i, counted GLOBALLY (it never decreases)
//     h[i]  c at the head of i's score group   (a head: key >> 1 differs from the predecessor's; a new group is a new score group,
//                                               so equal scores on both sides of a group boundary are no tie)
//     b[i]  c at the head of i's group         (a head: key >> 32 differs from the predecessor's)
// h and b are running maxima of c over the heads up to i.  A positive at i contributes (c[i] - b[i]) + (h[i] - b[i]) to its group's
// U2_g = sum over the group's positives of (2 #{the group's smaller negatives} + #{the group's equal negatives}).
// Per group: P_g, N_g, U2_g; the group is MIXED when P_g N_g > 0.  The host takes
//     GAUC = sum over mixed groups of n_g U2_g / (2 P_g N_g)  /  sum over mixed groups of n_g,     n_g = P_g + N_g
// from the integers (metrics.group_auc_from_records).  Every output word is an integer that depends on neither batch sizes, batch
// order nor the order threads run in.
//
// HOW A GROUP IS REDUCED.  With S[i] the exclusive prefix sum of the contributions, a group that starts at position s and whose
// last key is at position e has N_g = c[e + 1] - c[s], n_g = e + 1 - s and U2_g = S[e + 1] - S[s].  c, the position and S never
// decrease, so "the value at the head of my group" is a running maximum over the group heads for all three (b, q and sb below):
// the thread that holds a group's LAST key has everything the group needs, wherever the group started -- inside the tile, exactly
// on a tile edge, or several tiles back.
//
// KERNELS.  append (one launch per eval batch): keys at the slot the host names (groups read through an element stride, so
// ids[:, slot] of a [B, F] batch needs no copy), the batch's invalid count with one 64-bit integer atomic per workgroup.
// finalize:
//   zero         digit totals + the header
//   sort         csrc/auc_sort_device.h on the low 32 + group_bits bits: 4 + ceil(group_bits / 8) passes of { histogram ; scan ;
//                scatter }; an odd pass count starts from a copy, so the sorted keys end in the caller's buffer
//   counts       per tile: negatives, positives (one atomic per workgroup), local c at the last score head and at the last group
//                head, local position of the last group head
//   tile scan 0  ONE workgroup: exclusive negatives; exclusive running maxima -> h, b, q in front of every tile; header totals
//   pass 1       per tile: contributions; their sum and the local S at the tile's last group head
//   tile scan 1  exclusive S; exclusive running maximum -> sb in front of every tile
//   pass 2       per tile: every group tail's (P_g, N_g); groups and examples in one-class groups (one atomic each per workgroup),
//                mixed groups per tile
//   tile scan 2  exclusive mixed groups in front of every tile; their total into the header
// records (after the host has read the header): pass 3 = pass 2's arithmetic + one (g, P_g, N_g, U2_g) record per mixed group at
// slot = mixed groups in front of it, in ascending g.  Every store is guarded by the capacity.
// Every step that needs another workgroup's result is a kernel boundary: no grid barrier, no spin-wait, no look-back chain; inside
// a launch workgroups meet in integer atomics only.  Grids are bounded (AX_MAX_GRID workgroups stride over the tiles).
#include "rsx_common.h"
#include "auc_sort_device.h"
#include "eval_device.h"      // the example rule and the append kernel, the workgroup scans, the key predicates, the tile load

namespace {
constexpr int AG_MAX_PASSES = 8;        // 4 + ceil(31 / 8)
constexpr int AG_HDR = 8;               // header words (the last one is zero)

// ---- append: ev_append_k<uint64_t, true> of csrc/eval_device.h ----------------------------------------------------------------
__global__ __launch_bounds__(AX_T) void ag_zero_k(uint32_t* dtot, ull* hdr) {
  for (int i = threadIdx.x; i < AG_MAX_PASSES * AX_BINS; i += AX_T) dtot[i] = 0u;
  if (threadIdx.x < AG_HDR) hdr[threadIdx.x] = 0ull;
}

// ---- reduction over the sorted keys -------------------------------------------------------------------------------------------
struct AgRed {
  const uint64_t* keys;
  uint32_t* tneg;      // [nT]  counts: negatives of the tile                          -> scan 0: negatives in front of the tile
  uint32_t* thead;     // [nT]  counts: 1 + local c at the last score head (0: none)   -> scan 0: h in front of the tile
  uint32_t* tgrp;      // [nT]  counts: 1 + local c at the last group head             -> scan 0: b in front of the tile
  uint32_t* tq;        // [nT]  counts: 1 + local position of the last group head      -> scan 0: q in front of the tile
  uint32_t* tmix;      // [nT]  pass 2: mixed groups that end in the tile              -> scan 2: mixed groups in front of the tile
  ull* tU;             // [nT]  pass 1: contributions of the tile                      -> scan 1: S in front of the tile
  ull* tsb;            // [nT]  pass 1: 1 + local S at the last group head             -> scan 1: sb in front of the tile
  ull* hdr;            // {valid, invalid, groups, mixed groups, examples in one-class groups, P, N, 0}
  ull* rec;            // pass 3: [cap][4]
  ull cap;
  int n, nT;
};

struct AgTile : EvTile<uint64_t> {
  uint64_t next;       // the key behind k[3] (padding behind position n - 1: position n - 1 is a tail)
};

// thread tid holds the tile's keys 4 tid .. 4 tid + 3
__device__ __forceinline__ void ag_load_tile(const AgRed& a, int t, uint32_t* lds, AgTile& s) {
  const int i1 = t * AX_TILE + ((int)threadIdx.x + 1) * AX_IPL;
  s.next = i1 < a.n ? a.keys[i1] : ~0ull;
  ev_load_tile(a.keys, a.n, t, lds, s);
}

__global__ __launch_bounds__(AX_T) void ag_counts_k(const AgRed a) {
  __shared__ uint32_t l32[AX_W];
  const int tid = threadIdx.x;
  ull positives = 0ull;                                   // thread 0: over this workgroup's tiles
  for (int t = blockIdx.x; t < a.nT; t += gridDim.x) {
    AgTile s;
    ag_load_tile(a, t, l32, s);
    uint32_t run = s.excl, lh = 0u, lg = 0u, lq = 0u, pc = 0u;
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      const uint64_t pk = k == 0 ? s.prev : s.k[k - 1];
      if (ev_shead(s.k[k], pk)) lh = run + 1u;
      if (ev_ghead(s.k[k], pk)) {
        lg = run + 1u;
        lq = (uint32_t)(tid * AX_IPL + k) + 1u;
      }
      run += ev_neg(s.k[k]) ? 1u : 0u;
      pc += ev_pos(s.k[k]) ? 1u : 0u;
    }
    uint32_t mh, mg, mq, ptot;
    ev_block_excl<true, AX_W>(lh, l32, mh);
    ev_block_excl<true, AX_W>(lg, l32, mg);
    ev_block_excl<true, AX_W>(lq, l32, mq);
    ev_block_excl<false, AX_W>(pc, l32, ptot);
    if (tid == 0) {
      a.tneg[t] = s.total;
      a.thead[t] = mh;
      a.tgrp[t] = mg;
      a.tq[t] = mq;
      positives += ptot;
    }
  }
  if (tid == 0 && positives) atomicAdd(&a.hdr[5], positives);
}

// phase 0 (after counts): negatives in front of every tile; h, b and q in front of it (the running maxima of the tiles' last-head
// values made global: c and the position never decrease, so "the last" is "the largest"; 0 when there is none, which only the
// first tile sees, whose first key is a head itself); the header's totals.
// phase 1 (after pass 1): S in front of every tile and sb in front of it.      phase 2 (after pass 2): mixed groups in front.
__global__ __launch_bounds__(AX_T) void ag_scan_k(const AgRed a, int phase) {
  __shared__ uint32_t l32[AX_W];
  __shared__ ull l64[AX_W];
  if (phase == 0) {
    const uint32_t N = ev_tiles_scan<false, AX_W>(a.tneg, a.nT, l32, [](int, uint32_t v) { return v; });
    const auto to_c = [&](int t, uint32_t l) { return l ? a.tneg[t] + l - 1u : 0u; };
    ev_tiles_scan<true, AX_W>(a.thead, a.nT, l32, to_c);
    ev_tiles_scan<true, AX_W>(a.tgrp, a.nT, l32, to_c);
    ev_tiles_scan<true, AX_W>(a.tq, a.nT, l32, [](int t, uint32_t l) { return l ? (uint32_t)t * AX_TILE + l - 1u : 0u; });
    if (threadIdx.x == 0) {
      const ull P = a.hdr[5];
      a.hdr[6] = N;
      a.hdr[0] = P + N;
      a.hdr[1] = (ull)a.n - P - N;
    }
  } else if (phase == 1) {
    ev_tiles_scan<false, AX_W>(a.tU, a.nT, l64, [](int, ull v) { return v; });
    ev_tiles_scan<true, AX_W>(a.tsb, a.nT, l64, [&](int t, ull l) { return l ? a.tU[t] + l - 1ull : 0ull; });
  } else {
    const uint32_t M = ev_tiles_scan<false, AX_W>(a.tmix, a.nT, l32, [](int, uint32_t v) { return v; });
    if (threadIdx.x == 0) a.hdr[3] = M;
  }
}

// MODE 1: the tile's contributions and its local S at the last group head.   MODE 2: the groups that END in the tile, counted.
// MODE 3: the mixed ones among them, written.
template <int MODE>
__global__ __launch_bounds__(AX_T) void ag_pass_k(const AgRed a) {
  __shared__ uint32_t l32[AX_W];
  __shared__ ull l64[AX_W];
  const int tid = threadIdx.x;
  ull groups = 0ull, skipped = 0ull;                      // MODE 2: this thread's tails and their one-class examples
  const ull cap = MODE == 3 ? (a.cap < a.hdr[3] ? a.cap : a.hdr[3]) : 0ull;
  for (int t = blockIdx.x; t < a.nT; t += gridDim.x) {
    AgTile s;
    ag_load_tile(a, t, l32, s);
    const uint32_t p0 = (uint32_t)(t * AX_TILE + tid * AX_IPL);
    uint32_t c[AX_IPL];
    bool sh[AX_IPL], gh[AX_IPL];
    uint32_t run = a.tneg[t] + s.excl, hv = 0u, bv = 0u, qv = 0u;   // c / position at my last heads (0: none, the maximum's identity)
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      const uint64_t pk = k == 0 ? s.prev : s.k[k - 1];
      c[k] = run;
      sh[k] = ev_shead(s.k[k], pk);
      gh[k] = ev_ghead(s.k[k], pk);
      if (sh[k]) hv = run;
      if (gh[k]) {
        bv = run;
        qv = p0 + (uint32_t)k;
      }
      run += ev_neg(s.k[k]) ? 1u : 0u;
    }
    uint32_t m32;
    uint32_t ch = ev_block_excl<true, AX_W>(hv, l32, m32);
    uint32_t cb = ev_block_excl<true, AX_W>(bv, l32, m32);
    uint32_t cq = ev_block_excl<true, AX_W>(qv, l32, m32);
    ch = ev_op<true>(ch, a.thead[t]);
    cb = ev_op<true>(cb, a.tgrp[t]);
    cq = ev_op<true>(cq, a.tq[t]);
    ull con[AX_IPL], mine = 0ull;
    uint32_t bb[AX_IPL], qq[AX_IPL];
#pragma unroll
    for (int k = 0; k < AX_IPL; ++k) {
      if (sh[k]) ch = c[k];
      if (gh[k]) {
        cb = c[k];
        cq = p0 + (uint32_t)k;
      }
      bb[k] = cb;
      qq[k] = cq;
      con[k] = ev_pos(s.k[k]) ? (ull)(c[k] - cb) + (ull)(ch - cb) : 0ull;
      mine += con[k];
    }
    ull tot64;
    ull S = ev_block_excl<false, AX_W>(mine, l64, tot64);       // S of k[0]: local in MODE 1, global otherwise
    if (MODE != 1) S += a.tU[t];
    ull sv = 0ull;                                        // S at my last group head (MODE 1: + 1, 0 = none)
    {
      ull r = S;
#pragma unroll
      for (int k = 0; k < AX_IPL; ++k) {
        if (gh[k]) sv = MODE == 1 ? r + 1ull : r;
        r += con[k];
      }
    }
    ull m64;
    ull csb = ev_block_excl<true, AX_W>(sv, l64, m64);
    if (MODE == 1) {
      if (tid == 0) {
        a.tU[t] = tot64;
        a.tsb[t] = m64;
      }
    } else {
      csb = ev_op<true>(csb, a.tsb[t]);
      ull gP[AX_IPL], gN[AX_IPL], gU[AX_IPL];
      bool mixed[AX_IPL];
      uint32_t nmix = 0u;
      ull r = S;
#pragma unroll
      for (int k = 0; k < AX_IPL; ++k) {
        if (gh[k]) csb = r;
        mixed[k] = false;
        if (ev_gtail(s.k[k], k == AX_IPL - 1 ? s.next : s.k[k + 1])) {
          const uint32_t Ng = c[k] + (ev_neg(s.k[k]) ? 1u : 0u) - bb[k];
          const uint32_t ng = p0 + (uint32_t)k + 1u - qq[k];
          gN[k] = Ng;
          gP[k] = ng - Ng;
          gU[k] = r + con[k] - csb;
          mixed[k] = Ng != 0u && ng != Ng;
          if (MODE == 2) {
            groups += 1ull;
            skipped += mixed[k] ? 0ull : (ull)ng;
          }
          nmix += mixed[k] ? 1u : 0u;
        }
        r += con[k];
      }
      uint32_t tmixed;
      uint32_t slot = ev_block_excl<false, AX_W>(nmix, l32, tmixed);
      if (MODE == 2) {
        if (tid == 0) a.tmix[t] = tmixed;
      } else {
        slot += a.tmix[t];
#pragma unroll
        for (int k = 0; k < AX_IPL; ++k) {
          if (mixed[k]) {
            if ((ull)slot < cap) {
              ulonglong2* o = reinterpret_cast<ulonglong2*>(a.rec + 4ull * slot);
              o[0] = make_ulonglong2(s.k[k] >> 32, gP[k]);
              o[1] = make_ulonglong2(gN[k], gU[k]);
            }
            ++slot;
          }
        }
      }
    }
  }
  if (MODE == 2) {
    ull tg, ts;
    ev_block_excl<false, AX_W>(groups, l64, tg);
    ev_block_excl<false, AX_W>(skipped, l64, ts);
    if (tid == 0) {
      if (tg) atomicAdd(&a.hdr[2], tg);
      if (ts) atomicAdd(&a.hdr[4], ts);
    }
  }
}

inline int ag_passes(int group_bits) { return 4 + (group_bits + 7) / 8; }

// [second key buffer: 8 n, rounded up to 256] [histogram: 4 * 256 * nT | digit totals: 4 * 8 * 256 | 5 tile arrays: 4 * 5 * nT,
// together rounded up to 256] [2 tile arrays of 64-bit words: 16 * nT]
inline size_t ag_mid_bytes(size_t nT) { return ax_align((size_t)AX_BINS * nT * 4 + (size_t)AG_MAX_PASSES * AX_BINS * 4 + nT * 20); }
inline size_t ag_ws_bytes(int64_t n) {
  const size_t nT = ax_tiles(n);
  return ax_align((size_t)n * 8) + ag_mid_bytes(nT) + nT * 16;
}

struct AgCarve {
  uint64_t* alt;
  uint32_t* hist;
  uint32_t* dtot;
  AgRed r;
};

inline AgCarve ag_carve(uint64_t* keys, int64_t n, void* workspace, uint64_t* header) {
  AgCarve c;
  const size_t nT = ax_tiles(n);
  char* ws = static_cast<char*>(workspace);
  c.alt = reinterpret_cast<uint64_t*>(ws);
  c.hist = reinterpret_cast<uint32_t*>(ws + ax_align((size_t)n * 8));
  c.dtot = c.hist + (size_t)AX_BINS * nT;
  c.r.keys = keys;
  c.r.tneg = c.dtot + AG_MAX_PASSES * AX_BINS;
  c.r.thead = c.r.tneg + nT;
  c.r.tgrp = c.r.thead + nT;
  c.r.tq = c.r.tgrp + nT;
  c.r.tmix = c.r.tq + nT;
  c.r.tU = reinterpret_cast<ull*>(ws + ax_align((size_t)n * 8) + ag_mid_bytes(nT));
  c.r.tsb = c.r.tU + nT;
  c.r.hdr = reinterpret_cast<ull*>(header);
  c.r.rec = nullptr;
  c.r.cap = 0ull;
  c.r.n = (int)n;
  c.r.nT = (int)nT;
  return c;
}
}  // namespace

extern "C" int64_t rsx_auc_group_max_keys(void) { return AX_MAX_N; }

extern "C" size_t rsx_auc_group_workspace_bytes(int64_t n, int group_bits) {
  if (n < 0 || n > AX_MAX_N || group_bits < 1 || group_bits > 31) return 0;
  return ag_ws_bytes(n);
}

extern "C" int rsx_auc_group_append(const float* prob, const float* labels, const int32_t* groups, int64_t group_stride, int64_t n,
                                    int group_bits, uint64_t* keys_at_offset, uint64_t* invalid_word, rsx_stream_t stream) {
  if (!prob || !labels || !groups || !keys_at_offset || !invalid_word || n < 0 || n > AX_MAX_N) return RSX_EINVAL;
  if (group_bits < 1 || group_bits > 31 || group_stride < 1) return RSX_EINVAL;
  if (reinterpret_cast<uintptr_t>(keys_at_offset) & 7u) return RSX_EINVAL;
  if (n == 0) return RSX_OK;
  ev_append<uint64_t, true>(prob, labels, groups, group_stride, n, 1u << group_bits, keys_at_offset, invalid_word,
                            rsx_s(stream));
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}

extern "C" int rsx_auc_group_finalize(uint64_t* keys, int64_t n, int group_bits, void* workspace, size_t workspace_bytes,
                                      uint64_t* header, rsx_stream_t stream) {
  if (!keys || !workspace || !header || n < 0 || n > AX_MAX_N || group_bits < 1 || group_bits > 31) return RSX_EINVAL;
  if (workspace_bytes < ag_ws_bytes(n)) return RSX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(keys) & 15u) || (reinterpret_cast<uintptr_t>(workspace) & 15u) ||
      (reinterpret_cast<uintptr_t>(header) & 7u))
    return RSX_EINVAL;
  hipStream_t st = rsx_s(stream);
  AgCarve c = ag_carve(keys, n, workspace, header);
  RSX_LAUNCH(ag_zero_k, dim3(1), dim3(AX_T), 0, st, c.dtot, c.r.hdr);
  if (n == 0) {
    RSX_CHECK_LAUNCH();
    return RSX_OK;
  }
  ax_sort_passes<uint64_t>(keys, c.alt, c.hist, c.dtot, c.r.n, c.r.nT, ag_passes(group_bits), st);
  RSX_CHECK_LAUNCH();
  const unsigned grid = ax_grid(c.r.nT);
  RSX_LAUNCH(ag_counts_k, dim3(grid), dim3(AX_T), 0, st, c.r);
  RSX_LAUNCH(ag_scan_k, dim3(1), dim3(AX_T), 0, st, c.r, 0);
  RSX_LAUNCH(ag_pass_k<1>, dim3(grid), dim3(AX_T), 0, st, c.r);
  RSX_LAUNCH(ag_scan_k, dim3(1), dim3(AX_T), 0, st, c.r, 1);
  RSX_LAUNCH(ag_pass_k<2>, dim3(grid), dim3(AX_T), 0, st, c.r);
  RSX_LAUNCH(ag_scan_k, dim3(1), dim3(AX_T), 0, st, c.r, 2);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}

extern "C" int rsx_auc_group_records(const uint64_t* keys, int64_t n, const void* workspace, const uint64_t* header,
                                     uint64_t* records, int64_t record_capacity, rsx_stream_t stream) {
  if (!keys || !workspace || !header || n < 0 || n > AX_MAX_N || record_capacity < 0) return RSX_EINVAL;
  if (record_capacity > 0 && !records) return RSX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(keys) & 15u) || (reinterpret_cast<uintptr_t>(workspace) & 15u) ||
      (reinterpret_cast<uintptr_t>(header) & 7u) || (reinterpret_cast<uintptr_t>(records) & 15u))
    return RSX_EINVAL;
  if (n == 0 || record_capacity == 0) return RSX_OK;
  AgCarve c = ag_carve(const_cast<uint64_t*>(keys), n, const_cast<void*>(workspace), const_cast<uint64_t*>(header));
  c.r.rec = reinterpret_cast<ull*>(records);
  c.r.cap = (ull)record_capacity;
  RSX_LAUNCH(ag_pass_k<3>, dim3(ax_grid(c.r.nT)), dim3(AX_T), 0, rsx_s(stream), c.r);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
