// TF-1.x Adam sweep as device/host building blocks shared by adam.hip (the stand-alone launch) and tower.hip (where
// slices of the untouched-row sweep ride along in the tower launches).  See adam.hip for the semantics.
#pragma once
#include "adam_fast.h"
#include "rsx_common.h"

struct SegDev {
  int32_t kind, d;
  long long n;
  float *var, *m, *v, *g;
  const int32_t *slot, *uniq_row, *nuniq;
  int32_t B, stride, zero_grad;
  uint32_t blk_begin;
  int32_t g_rep, g_rep_stride4;      // *_ROWS kinds: replicas of g summed in order, float4 units apart (rsx_adam_seg.g_replicas)
};
constexpr int ADAM_WMAX = RSX_ADAM_WINDOW_MAX - 1;     // extra slot maps of an optimizer window
struct AdamArgs {
  SegDev seg[RSX_ADAM_MAX_SEGS];
  // *_COLD kinds of an optimizer WINDOW (rsx_adam_seg.slot_w): the slot maps of the window's later steps, shared by every COLD
  // segment of the launch (kernel arguments are limited to 4 KB and a launch may embed two AdamArgs)
  // -- equally spaced (one allocation; base + stride keeps them out of the scalar registers)
  const int32_t* slot_w0;
  long long slot_w_stride;      // in int32 elements
  int32_t nw;
  int32_t nseg;
  float lr, b1, b2, eps;
  float* state;
  uint32_t total_blocks;
  // Window sweeps that RIDE in the steps' launches, a slice per step (round 4, rsx_adam_slice.window_block_u / alphas_from_state):
  // win_u = float4 per lane of a TABLE_TF1_COLD block (0: ADAM_U) -- smaller blocks spread a slice over the idle CUs of a
  // latency-bound launch --; alpha_src != 0: the window's step sizes are READ from state words 8.. (the slice of the window's
  // first step computed them from the beta powers, which later steps have advanced since).
  int32_t win_u, alpha_src;
};

struct Hp {
  float alpha, b1, b2, omb1, omb2, eps;
};

__device__ __forceinline__ void adam_sparse1(float& var, float& m, float& v, float g, bool has, const Hp& h) {
  float m1 = m * h.b1;
  float v1 = v * h.b2;
  if (has) {
    m1 = m1 + g * h.omb1;
    v1 = v1 + (g * g) * h.omb2;
  }
  var = var - (h.alpha * m1) / (sqrtf(v1) + h.eps);
  m = m1;
  v = v1;
}
__device__ __forceinline__ void adam_dense1(float& var, float& m, float& v, float g, const Hp& h) {
  const float m1 = m + (g - m) * h.omb1;
  const float v1 = v + (g * g - v) * h.omb2;
  var = var - (m1 * h.alpha) / (sqrtf(v1) + h.eps);
  m = m1;
  v = v1;
}

#define F4_APPLY(FN, VAR, M, V, G, ...)   \
  FN(VAR.x, M.x, V.x, G.x, __VA_ARGS__);  \
  FN(VAR.y, M.y, V.y, G.y, __VA_ARGS__);  \
  FN(VAR.z, M.z, V.z, G.z, __VA_ARGS__);  \
  FN(VAR.w, M.w, V.w, G.w, __VA_ARGS__)

#ifndef RSX_ADAM_U
#define RSX_ADAM_U 8
#endif
#ifndef RSX_ADAM_NT
#define RSX_ADAM_NT 0
#endif
#ifndef RSX_ADAM_WIN_HB
#define RSX_ADAM_WIN_HB 2      // float4 per lane and pipeline stage of the window sweep (adam_window_block)
#endif
constexpr int ADAM_T = 256;         // threads per workgroup
constexpr int ADAM_U = RSX_ADAM_U;  // float4 per lane
constexpr long long ADAM_Q = (long long)ADAM_T * ADAM_U;  // float4 per workgroup
// DENSE segments take 2 float4 per lane: a dense arena is small (0.3 MB for DeepFM) and rides in the latency-bound scatter
// launch, where 8 sequential IEEE div + sqrt updates per lane (~1 900 instructions of one wave) made its 9 workgroups the
// LAST ones to finish (stamps: 8.6 us after the launch's first workgroup, against 4.8 for the window pass).
constexpr int ADAM_U_DENSE = 2;
constexpr long long ADAM_Q_DENSE = (long long)ADAM_T * ADAM_U_DENSE;
// VEC_COLD segments of a WINDOW sweep in full-size blocks (nw > 0, win_u == 0: the stand-alone launch, adam_window_k) take 2
// float4 per lane as well: the first-order vector is 1 / 16 of the tables' elements, but each of its elements takes the
// 1 + nw updates one by one (adam_window_vec_block), and in 2 048-float4 blocks DeepFM's vector was 103 workgroups of the
// launch's 1 861 that ran as long as the whole launch.  411 workgroups spread the same work over every CU.
constexpr int ADAM_U_WVEC = 2;
constexpr long long ADAM_Q_WVEC = (long long)ADAM_T * ADAM_U_WVEC;
// float4 positions per lane of a VEC_SLOT / VEC_COLD block (host and device: adam_build_args lays the blocks out with it)
__host__ __device__ __forceinline__ int adam_vec_u(const int kind, const int nw, const int win_u) {
  return kind == RSX_ADAM_VEC_COLD && nw > 0 && win_u == 0 ? ADAM_U_WVEC : ADAM_U;
}

// "Am I the last workgroup of this launch?" for thread 0 of every workgroup, after its block's work (and a __syncthreads):
// arrival counters by workgroup index modulo 32 (one 128-byte line each: state words 4 + 32 r), then the shared ticket
// (state word 2) for the last arrival of each residue.  All counters are left at zero.  total = workgroups of the launch.
__device__ __forceinline__ bool adam_arrive_last(float* state, const uint32_t total) {
  uint32_t* w = reinterpret_cast<uint32_t*>(state);
  const uint32_t r = blockIdx.x & 31u;
  const uint32_t n_r = (total + 31u - r) >> 5;                  // workgroups with this residue
  uint32_t* sub = w + 4 + 32 * r;
  if (atomicAdd(sub, 1u) != n_r - 1u) return false;
  *sub = 0u;
  const uint32_t n_top = total < 32u ? total : 32u;             // residues in use
  if (atomicAdd(w + 2, 1u) != n_top - 1u) return false;
  w[2] = 0u;
  return true;
}

// alpha of the window's later steps: step j of the window runs with the beta powers advanced j times -- the same fp32
// products the per-step advance of the powers makes.  (Named scalars, no array: a dynamically indexed local array is
// promoted to LDS / scratch by this toolchain.)
struct AlphaW {
  float a0, a1, a2, a3, a4, a5, a6;
  __device__ __forceinline__ float get(int j) const {
    return j == 0 ? a0 : j == 1 ? a1 : j == 2 ? a2 : j == 3 ? a3 : j == 4 ? a4 : j == 5 ? a5 : a6;
  }
};
static_assert(ADAM_WMAX == 7, "AlphaW holds 7 steps");
__device__ __forceinline__ AlphaW alpha_window(const AdamArgs& a, int nw, float b1p, float b2p) {
  AlphaW aw = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (nw > 0) {
    float p1 = b1p, p2 = b2p;
#define RSX_ALPHA_NEXT(dst) p1 *= a.b1; p2 *= a.b2; dst = a.lr * sqrtf(1.0f - p2) / (1.0f - p1)
    RSX_ALPHA_NEXT(aw.a0); RSX_ALPHA_NEXT(aw.a1); RSX_ALPHA_NEXT(aw.a2); RSX_ALPHA_NEXT(aw.a3);
    RSX_ALPHA_NEXT(aw.a4); RSX_ALPHA_NEXT(aw.a5); RSX_ALPHA_NEXT(aw.a6);
#undef RSX_ALPHA_NEXT
  }
  return aw;
}

// The step sizes of a sweep over 1 + nw steps: from the beta powers (state words 0, 1), or -- a slice of a window sweep that runs
// at a LATER step of its window -- the values the window's first slice left in state words 8.. (the same floats).
__device__ __forceinline__ void adam_step_sizes(const AdamArgs& a, int nw, float& alpha0, AlphaW& aw) {
  if (a.alpha_src) {
    alpha0 = a.state[8];
    aw = AlphaW{a.state[9], a.state[10], a.state[11], a.state[12], a.state[13], a.state[14], a.state[15]};
    return;
  }
  const float b1p = a.state[0], b2p = a.state[1];
  alpha0 = a.lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
  aw = alpha_window(a, nw, b1p, b2p);
}
// The step sizes of the window's 1 + NW steps, for the lazy window pass of segsum_adam_k (csrc/embedding.hip), which applies
// a row's zero-gradient updates of several steps -- also FUTURE ones -- in one go: state word 8 + j = the step size of
// window step j, from the products the per-step advance of the beta powers will make.  ONE thread of the window's first sweep
// launch (or first slice) calls this.
template <int NW>
__device__ __forceinline__ void adam_publish_step_sizes(const AdamArgs& a) {
  const float b1p = a.state[0], b2p = a.state[1];
  const AlphaW aw = alpha_window(a, NW, b1p, b2p);
  a.state[8] = a.lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
#pragma unroll
  for (int j = 0; j < NW; ++j) a.state[9 + j] = aw.get(j);
}

// One workgroup (ADAM_T = 256 threads) of the sweep: block `blk` of the launch-wide block index space of `a`.
__device__ __forceinline__ void adam_block(const AdamArgs& a, const uint32_t blk, const int tid = threadIdx.x) {
  Hp h;
  h.b1 = a.b1;
  h.b2 = a.b2;
  h.omb1 = 1.0f - a.b1;
  h.omb2 = 1.0f - a.b2;
  h.eps = a.eps;
  int si = 0;
#pragma unroll 1
  for (int k = 1; k < a.nseg; ++k)
    if (blk >= a.seg[k].blk_begin) si = k;
  const SegDev& s = a.seg[si];
  // window of 1 + nw steps (COLD kinds only): step j of the window runs with the beta powers advanced j times -- the same
  // fp32 products the per-step advance of the powers makes
  const bool is_cold = s.kind == RSX_ADAM_TABLE_TF1_COLD || s.kind == RSX_ADAM_VEC_COLD;
  const int nw = is_cold ? a.nw : 0;
  AlphaW aw;
  adam_step_sizes(a, nw, h.alpha, aw);
  // the window's extra slot maps are equally spaced (one allocation): base + stride instead of 7 pointers in scalar registers
  const int32_t* __restrict__ swb = a.slot_w0;
  const long long sws = a.slot_w_stride;
  const int vec_u = adam_vec_u(s.kind, a.nw, a.win_u);        // (ADAM_U for every kind but a window's VEC_COLD)
  const long long base = (long long)(blk - s.blk_begin) * (s.kind == RSX_ADAM_DENSE ? ADAM_Q_DENSE : (long long)ADAM_T * vec_u);
  float4* __restrict__ var4 = reinterpret_cast<float4*>(s.var);
  float4* __restrict__ m4 = reinterpret_cast<float4*>(s.m);
  float4* __restrict__ v4 = reinterpret_cast<float4*>(s.v);

  if (s.kind == RSX_ADAM_TABLE_TF1 || s.kind == RSX_ADAM_TABLE_TF1_COLD) {
    const bool cold_only = s.kind == RSX_ADAM_TABLE_TF1_COLD;   // touched rows are left to the TABLE_ROWS launch
    const int lpr = s.d >> 2;
    const long long n4 = s.n * lpr;
    const float4* __restrict__ G4 = reinterpret_cast<const float4*>(s.g);
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) {
      const long long e = base + (long long)u * ADAM_T + tid;
      if (e < n4) {
        const long long row = e / lpr;
        const int q = (int)(e - row * lpr);
        int sl = s.slot[row];
        for (int l = 0; l < nw; ++l) sl &= swb[(long long)l * sws + row];      // window (see adam_window_block for the fast form)
        if (cold_only && sl >= 0) continue;
#if RSX_ADAM_NT
        float4 var = __builtin_nontemporal_load(&var4[e]), m = __builtin_nontemporal_load(&m4[e]),
               v = __builtin_nontemporal_load(&v4[e]);
#else
        float4 var = var4[e], m = m4[e], v = v4[e];
#endif
        const bool has = sl >= 0;
        const float4 g = has ? G4[(long long)sl * lpr + q] : F4Z;
        F4_APPLY(adam_sparse1, var, m, v, g, has, h);
#pragma unroll 1
        for (int j = 0; j < nw; ++j) {
          Hp hj = h;
          hj.alpha = aw.get(j);
          F4_APPLY(adam_sparse1, var, m, v, F4Z, false, hj);
        }
#if RSX_ADAM_NT
        __builtin_nontemporal_store(var, &var4[e]);
        __builtin_nontemporal_store(m, &m4[e]);
        __builtin_nontemporal_store(v, &v4[e]);
#else
        var4[e] = var;
        m4[e] = m;
        v4[e] = v;
#endif
      }
    }
  } else if (s.kind == RSX_ADAM_DENSE) {
    float4* __restrict__ g4 = reinterpret_cast<float4*>(s.g);
    const long long n4 = s.n >> 2;
    // B > 1: the gradient is the sum of B replicas' arenas, `stride` floats apart inside an all-gathered buffer, added in
    // rank order (every rank computes the same bits) -- the data-parallel dense all-reduce folded into the update
    const int nrep = s.B > 1 ? s.B : 1;
    const long long rs4 = (long long)s.stride >> 2;
#pragma unroll
    for (int u = 0; u < ADAM_U_DENSE; ++u) {
      const long long e = base + (long long)u * ADAM_T + tid;
      if (e < n4) {
        float4 var = var4[e], m = m4[e], v = v4[e];
        float4 g = g4[e];
        int r = 1;
        // (many replicas -- fm.py's per-example head gradients, round 4: 16 loads in flight per trip; the same ascending order)
        for (; r + 15 < nrep; r += 16) {
          float4 t[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) t[q] = g4[e + (long long)(r + q) * rs4];
#pragma unroll
          for (int q = 0; q < 16; ++q) { g.x += t[q].x; g.y += t[q].y; g.z += t[q].z; g.w += t[q].w; }
        }
        for (; r < nrep; ++r) {
          const float4 gr = g4[e + r * rs4];
          g.x += gr.x; g.y += gr.y; g.z += gr.z; g.w += gr.w;
        }
        F4_APPLY(adam_dense1, var, m, v, g, h);
        var4[e] = var;
        m4[e] = m;
        v4[e] = v;
        if (s.zero_grad) g4[e] = F4Z;
      } else if (e == n4) {  // scalar tail (n not a multiple of 4)
        for (long long i = n4 * 4; i < s.n; ++i) {
          float g = s.g[i];
          for (int r = 1; r < nrep; ++r) g += s.g[i + (long long)r * s.stride];
          adam_dense1(s.var[i], s.m[i], s.v[i], g, h);
          if (s.zero_grad) s.g[i] = 0.f;
        }
      }
    }
  } else if (s.kind == RSX_ADAM_VEC_SLOT || s.kind == RSX_ADAM_VEC_COLD) {
    const bool cold_only = s.kind == RSX_ADAM_VEC_COLD;         // touched elements keep their state for VEC_ROWS_DENSE
    const long long n4 = s.n >> 2;
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) {
      const long long e = u < vec_u ? base + (long long)u * ADAM_T + tid : n4 + 1;      // (positions past a short block: no-ops)
      if (e < n4) {
        int4 sl = reinterpret_cast<const int4*>(s.slot)[e];
        for (int l = 0; l < nw; ++l) {
          const int4 t = reinterpret_cast<const int4*>(swb + (long long)l * sws)[e];
          sl.x &= t.x; sl.y &= t.y; sl.z &= t.z; sl.w &= t.w;
        }
        float4 g;
        g.x = (!cold_only && sl.x >= 0) ? s.g[sl.x] : 0.f;     // COLD: g is not provided (touched elements are restored below)
        g.y = (!cold_only && sl.y >= 0) ? s.g[sl.y] : 0.f;
        g.z = (!cold_only && sl.z >= 0) ? s.g[sl.z] : 0.f;
        g.w = (!cold_only && sl.w >= 0) ? s.g[sl.w] : 0.f;
        float4 var = var4[e], m = m4[e], v = v4[e];
        const float4 var0 = var, m0 = m, v0 = v;
        F4_APPLY(adam_dense1, var, m, v, g, h);
        for (int j = 0; j < nw; ++j) {
          Hp hj = h;
          hj.alpha = aw.get(j);
          F4_APPLY(adam_dense1, var, m, v, F4Z, hj);
        }
        if (cold_only) {   // element-wise: leave the touched elements exactly as they were
          if (sl.x >= 0) { var.x = var0.x; m.x = m0.x; v.x = v0.x; }
          if (sl.y >= 0) { var.y = var0.y; m.y = m0.y; v.y = v0.y; }
          if (sl.z >= 0) { var.z = var0.z; m.z = m0.z; v.z = v0.z; }
          if (sl.w >= 0) { var.w = var0.w; m.w = m0.w; v.w = v0.w; }
        }
        var4[e] = var;
        m4[e] = m;
        v4[e] = v;
      } else if (e == n4) {
        for (long long i = n4 * 4; i < s.n; ++i) {
          int sl = s.slot[i];
          for (int l = 0; l < nw; ++l) sl &= swb[(long long)l * sws + i];
          if (cold_only && sl >= 0) continue;
          adam_dense1(s.var[i], s.m[i], s.v[i], sl >= 0 ? s.g[sl] : 0.f, h);
          for (int j = 0; j < nw; ++j) {
            Hp hj = h;
            hj.alpha = aw.get(j);
            adam_dense1(s.var[i], s.m[i], s.v[i], 0.f, hj);
          }
        }
      }
    }
  } else if (s.kind == RSX_ADAM_TABLE_ROWS) {
    // lazy_rows mode: n = F*B slots, lpr lanes per slot; only listed rows move (NOT TF semantics)
    const int lpr = s.d >> 2;
    const long long n4 = s.n * lpr;
    const float4* __restrict__ G4 = reinterpret_cast<const float4*>(s.g);
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) {
      const long long e = base + (long long)u * ADAM_T + tid;
      if (e < n4) {
        const long long sidx = e / lpr;
        const int q = (int)(e - sidx * lpr);
        const int f = (int)(sidx / s.B), j = (int)(sidx - (long long)f * s.B);
        if (j < s.nuniq[f]) {
          const long long sl = (long long)f * s.stride + j;
          const long long r = (long long)s.uniq_row[sl] * lpr + q;
          float4 var = var4[r], m = m4[r], v = v4[r];
          float4 g = G4[sl * lpr + q];
          for (int rr = 1; rr < s.g_rep; ++rr) g = f4_add(g, G4[(long long)rr * s.g_rep_stride4 + sl * lpr + q]);   // replicas, in rank order
          F4_APPLY(adam_sparse1, var, m, v, g, true, h);
          var4[r] = var;
          m4[r] = m;
          v4[r] = v;
        }
      }
    }
  } else {  // RSX_ADAM_VEC_ROWS (sparse formula) / RSX_ADAM_VEC_ROWS_DENSE (ApplyAdam formula)
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) {
      const long long sidx = base + (long long)u * ADAM_T + tid;
      if (sidx < s.n) {
        const int f = (int)(sidx / s.B), j = (int)(sidx - (long long)f * s.B);
        if (j < s.nuniq[f]) {
          const long long sl = (long long)f * s.stride + j;
          const int r = s.uniq_row[sl];
          float g = s.g[sl];
          for (int rr = 1; rr < s.g_rep; ++rr) g += s.g[(long long)rr * 4 * s.g_rep_stride4 + sl];
          if (s.kind == RSX_ADAM_VEC_ROWS_DENSE) adam_dense1(s.var[r], s.m[r], s.v[r], g, h);
          else adam_sparse1(s.var[r], s.m[r], s.v[r], g, true, h);
        }
      }
    }
  }
}

#ifndef RSX_ADAM_WIN_FAST
#define RSX_ADAM_WIN_FAST 1
#endif

// ---- scalar zero-gradient update (the first-order vector's rows in the lazy window pass of segsum_adam_k) ----------------
// adam_fast.h's sequences on ONE element, behind a guard on the operands themselves (checked after they have been computed):
// v1 in the square root's domain -- or +0 together with a +0 numerator, where both forms give var - (+0) --, numerator and
// denominator in the division's.  A wave with an active element outside takes the IEEE form for this update.
__device__ __forceinline__ float rsx_sqrt1_fast(const float x) {
  const float r = __builtin_amdgcn_rsqf(x), g = x * r, hh = r * 0.5f;
  return __builtin_fmaf(__builtin_fmaf(-g, g, x), hh, g);
}
__device__ __forceinline__ float rsx_div1_fast(const float n, const float d) {
  float r = __builtin_amdgcn_rcpf(d);
  r = __builtin_fmaf(__builtin_fmaf(-d, r, 1.f), r, r);
  const float q = n * r;
  return __builtin_fmaf(__builtin_fmaf(-d, q, n), r, q);
}
template <bool DENSE>
__device__ __forceinline__ void adam_zero_grad1(float& var, float& m, float& v, const bool active, const Hp& h) {
  float m1, v1, n;
  if constexpr (DENSE) {                      // adam_dense1 with g = 0, operation by operation
    m1 = m + (0.f - m) * h.omb1;
    v1 = v + (0.f * 0.f - v) * h.omb2;
    n = m1 * h.alpha;
  } else {                                    // adam_sparse1 with has = false
    m1 = m * h.b1;
    v1 = v * h.b2;
    n = h.alpha * m1;
  }
  const bool vz = __float_as_uint(v1) == 0u && __float_as_uint(n) == 0u;
  const float d = (vz ? 0.f : rsx_sqrt1_fast(vz ? 1.f : v1)) + h.eps;
  const uint32_t vb = __float_as_uint(v1), nb = __float_as_uint(n), na = nb & 0x7fffffffu, db = __float_as_uint(d);
  constexpr uint32_t V_LO = (127u - 96u) << 23, V_HI = (127u + 41u) << 23;      // rsx_sqrt2_fast: 2^-96 <= v1 < 2^41
  constexpr uint32_t D_LO = (127u - 30u) << 23, D_HI = (127u + 21u) << 23;      // rsx_div2_fast:  2^-30 <= d <= 2^21
  constexpr uint32_t N_LO = (127u - 94u) << 23, N_HI = (127u + 34u) << 23;      //                 n == +0 or 2^-94 <= |n| <= 2^34
  const bool ok = (vz || (vb - V_LO) < (V_HI - V_LO)) && (db - D_LO) <= (D_HI - D_LO) &&
                  (nb == 0u || (na - N_LO) <= (N_HI - N_LO));
  if (RSX_ADAM_WIN_FAST && __builtin_amdgcn_ballot_w64(active && !ok) == 0ull) {
    if (active) {
      var = var - rsx_div1_fast(n, d);
      m = m1;
      v = v1;
    }
  } else if (active) {
    if constexpr (DENSE) adam_dense1(var, m, v, 0.f, h);
    else adam_sparse1(var, m, v, 0.f, false, h);
  }
}

// ---- window sweep: packed fast form of the zero-gradient update --------------------------------------------------------

// One zero-gradient TF-1 update of two elements -- adam_sparse1(has = false) -- with the packed square root / division.
__device__ __forceinline__ void adam_zero_grad2(rsx_f2& var, rsx_f2& m, rsx_f2& v, const float alpha, const Hp& h) {
  m = m * h.b1;
  v = v * h.b2;
  const rsx_f2 n = m * alpha;
  const rsx_f2 d = rsx_sqrt2_fast(v) + h.eps;
  var = var - rsx_div2_fast(n, d);
}
// Does this element leave the domain on which the packed form returns the bits of the IEEE form, at any of the window's
// 1 + NW updates?  (Evaluated once per window on the loaded state; m and v only decay inside a window.)
//   v:  2^-86 <= v <= 2^40                            -> every v_j in [2^-94, 2^40], d_j = sqrt(v_j) + eps in [2^-30, 2^21]
//       v == +0 with m == +0 (a row no gradient has reached yet): the sweep computes with 1 in place of v -- n_j = +0, so
//       the quotient is +0 whatever the denominator -- and stores the zero back (adam_window_block)
//   m:  m_lo <= |m| <= 2^30 (m_lo = 2^-90 / min alpha) -> every n_j = alpha_j m_j has 2^-92 <= |n_j| <= 2^34: inside both domains
//       m == +0                                        -> n_j = +0, both forms return +0
//       |m| < m_lo (denormals, -0: where the moments of a row end up ~900 steps after its last gradient) and |var| >= 2^-24
//                                                      -> |n_j| < 2^-88, so |q_j| < 2^-56 in EITHER form (d_j >= 2^-30; the
//                                                         fast chain's result is bounded by 3 |n_j| / d_j): var - q_j == var
// Anything else (NaN / inf moments, a tiny moment under a tiny weight, v below 2^-86) sends the wave to the IEEE form.
__device__ __forceinline__ bool adam_win_guard1(const float var, const float m, const float v, const uint32_t m_lo_bits) {
  const uint32_t vb = __float_as_uint(v), mb = __float_as_uint(m), ma = mb & 0x7fffffffu;
  const uint32_t va = __float_as_uint(var) & 0x7fffffffu;
  constexpr uint32_t V_LO = (127u - 86u) << 23, V_HI = (127u + 40u) << 23, M_HI = (127u + 30u) << 23;
  constexpr uint32_t VAR_LO = (127u - 24u) << 23;
  const bool v_ok = (vb - V_LO) <= (V_HI - V_LO);
  const bool m_mid = (ma - m_lo_bits) <= (M_HI - m_lo_bits);
  const bool m_tiny = ma < m_lo_bits && va >= VAR_LO;
  return !(mb == 0u ? (v_ok || vb == 0u) : (v_ok && (m_mid || m_tiny)));
}
__device__ __forceinline__ bool adam_win_guard4(const float4& var, const float4& m, const float4& v, const uint32_t m_lo_bits) {
  return adam_win_guard1(var.x, m.x, v.x, m_lo_bits) | adam_win_guard1(var.y, m.y, v.y, m_lo_bits) |
         adam_win_guard1(var.z, m.z, v.z, m_lo_bits) | adam_win_guard1(var.w, m.w, v.w, m_lo_bits);
}

// The untouched rows of a window of 1 + NW steps (its own kernel, adam_window_k: the packed forms' temporaries would
// otherwise count against every carrier kernel and the one-step sweep, which inherit adam_block's 61 registers).
//   - TABLE_TF1_COLD blocks: batches of HB float4 per lane in phases, so that every load of a batch is in flight before
//     the first use: slot maps (clamped index), then var / m / v unconditionally (a skipped row costs its read, ~1 % of the
//     traffic; a guarded load would serialise the batch), then the 1 + NW updates, then the stores of the rows that moved.
//     Software pipeline over the block's NB batches: the loads of batch b + 1 are issued before batch b is updated.
//     (Measured against it at 8 / 4 steps per window, us per sweep of the DeepFM state: this form 86.5 / 61.0; persistent
//     workgroups walking batches with a stride of the grid 85.2 / 64.7 at 4 per CU, 81.0 / 59.9 at 8 per CU; one batch per
//     workgroup without a pipeline 97.5 / 65.6.  With the state L2-resident the updates alone cost ~9 us per step of the
//     window: from ~4 steps per window on the kernel is VALU-bound, not HBM-bound.)
//   - VEC_COLD blocks of the stand-alone sweep (U == ADAM_U): adam_window_vec_block, below.
//   - blocks of the other kinds, and the riders' VEC_COLD blocks: adam_block.
// U = float4 per lane of a block (== a.win_u, or ADAM_U when that is 0: the host picks the instantiation)
//
// COMPACT (rsx_adam_slice.window_compact; the stand-alone sweep only, rows of 4 .. 256 floats, a power of two): a row whose m
// is +0 throughout receives var - (+0) from every update -- var keeps its bits, m stays +0, and v only takes its 1 + NW
// products with b2 -- so the chain runs on the other rows only, and on FULL waves of them:
//   phase 1  slot maps, m and v of the block (not var), the same pipeline.  The lanes of a row vote (ballots):
//              void  m and v all 0x00000000:                                       nothing more is loaded, nothing is stored
//              idle  m all 0x00000000, every v in [+0, +inf] (sign clear, no NaN): v = v * b2, 1 + NW times, stored; var and
//                    m are neither loaded nor stored
//              live  every other untouched row: its float4s' offsets go to a list in LDS (ballot + mbcnt, one counter bump per
//                    wave and batch)
//   phase 2  the list, densely: 64 * HB entries per wave and batch, var / m / v loaded by index (m and v again, from the
//            cache), then finish() as it is -- guard, packed chain, IEEE redo.  At most one wave of the workgroup is partly
//            filled; waves beyond the list's end do nothing.
//   A wave whose first batch holds nothing but live rows (and skipped ones) classifies no further: it lists nothing and
//   runs the one-pass pipeline over its lanes of the block instead (after phase 2), which is right for rows of any class.
// The shortcuts hold under a launch-uniform gate on the hyper-parameters (win_shortcut_gate: otherwise every untouched row
// is live and 0 / 0, 0 * inf give the NaNs of the IEEE form).  Each launch derives every row's class from what it loads.
// (Not a bit of difference for any state arithmetic produces; a SIGNALLING NaN weight under an all-zero m keeps its payload
// here where var - 0 would quiet it.)
constexpr int WIN_LIST_WORDS = ADAM_T * ADAM_U + 1;     // the list of live float4s (offsets in the block) and its length
// May the compact form take a row with m == +0 throughout as one whose var does not move?  m * b1 = +0, alpha_j * (+0) = +0,
// v * b2 stays in [+0, +inf], sqrt + eps in (0, +inf], (+0) / that = +0, var - (+0) = var: finite hyper-parameters WITHOUT a
// sign (a negative b1 or step size makes the numerator -0, and -0 - (-0) = +0), b2 and eps above zero (inf * 0, 0 / 0).
template <int NW>
__device__ __forceinline__ bool win_shortcut_gate(const AdamArgs& a, const float alpha0, const AlphaW& aw) {
  auto plus_finite = [](const float x) { return __float_as_uint(x) < 0x7f800000u; };      // +0 .. FLT_MAX
  bool ok = plus_finite(a.eps) && a.eps > 0.f && plus_finite(a.b1) && plus_finite(a.b2) && a.b2 > 0.f && plus_finite(alpha0);
#pragma unroll
  for (int j = 0; j < NW; ++j) ok = ok && plus_finite(aw.get(j));
  return ok;
}
// Packed fast form of the zero-gradient updates (adam_fast.h), for the tables' and the vector's chain alike: usable (fast_ok)
// when the hyper-parameters keep every operand of a guarded element inside the fast forms' domains for all 1 + NW updates
// (b1^8 >= 1/4, b2^8 >= 2^-8, alphas within 4x).  Returns adam_win_guard1's lower bound on |m|, 2^-90 / min alpha, as bits.
template <int NW>
__device__ __forceinline__ uint32_t win_fast_form(const AdamArgs& a, const float alpha0, const AlphaW& aw, bool& fast_ok) {
  float amin = alpha0, amax = alpha0;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    amin = fminf(amin, aw.get(j));
    amax = fmaxf(amax, aw.get(j));
  }
  fast_ok = RSX_ADAM_WIN_FAST && a.b1 >= 0.85f && a.b1 < 1.f && a.b2 >= 0.5f && a.b2 < 1.f && a.eps >= 0x1p-30f &&
            a.eps <= 1.f && amin >= 0x1p-24f && amax <= 16.f && amax <= 4.f * amin;
  return __float_as_uint(fast_ok ? 0x1p-90f / amin : 1.f);
}

// ---- window sweep: the first-order vector (VEC_COLD blocks of the stand-alone launch, ADAM_U_WVEC float4 per lane) ------------
// adam_block's VEC_COLD branch gives every element -- void ones included -- 1 + NW IEEE adam_dense1 updates after ~10 dependent
// round trips per float4 (segment fields, slot map, one trip per window map, state), 8 float4 one after another, and stores all
// of them back: 103 workgroups that left 16 us after the last of the launch's 1 642 table blocks.  Here:
//   - the segment's fields are read once; every load of the block's 2 float4 per lane (slot map, the NW window maps, m, v,
//     var; unconditional, clamped index) is issued before the first use: one round trip;
//   - elements some step of the window touches (AND of the maps >= 0) are neither computed nor stored;
//   - under the launch-uniform gate (win_shortcut_gate, and 1 - b1, 1 - b2 in [+0, FLT_MAX]; with b2 > 0 that is 1 - b2 in
//     [0, 1)) an element with m = 0x00000000 and v in [+0, +inf) is STILL:  m1 = +0 + (0 - 0) omb1 = +0,
//     n = (+0) alpha = +0, v1 = v + (0 - v) omb2 = v - fl(v omb2) in [+0, v] (x - x = +0 in round-to-nearest), sqrt(v1) + eps
//     in (0, FLT_MAX], (+0) / that = +0, var - (+0) = var with all its bits.  void (v = +0 too): nothing moves, nothing is
//     stored.  idle: v alone takes its 1 + NW steps v + (0 - v) omb2 and is stored alone.  (v = +inf is NOT idle in this
//     formula, unlike the tables' v * b2: inf + (0 - inf) omb2 = NaN, which the next update carries into var.  m = -0 is live:
//     -0 + (0 - -0) omb1 = +0.)  The one non-arithmetic difference is the tables': a signalling NaN weight under a still element
//     keeps its payload;
//   - every other untouched element is live.  A wave whose live elements all pass adam_win_guard1 (once per window, on the
//     loaded state) takes the packed chain, adam_zero_grad2_dense, two elements per instruction; any other wave takes
//     adam_zero_grad1<true> 1 + NW times: adam_dense1(g = 0) operation by operation with the fast square root / division
//     behind a guard on each update's own operands, IEEE for a wave with an element outside;
//   - the math is skipped where no lane of the wave needs it; a float4 is stored when one of its elements moved (the others
//     return the bits that were loaded -- as adam_block does for touched elements).
// No compaction: with 2 float4 per lane the packed chain is well under 1 k instructions per wave, spread over 1 644 waves.
struct WinVecEl {
  float var, m, v;
  bool live, idle;
};
__device__ __forceinline__ void win_vec_classify(WinVecEl& x, const bool untouched, const bool gate) {
  const uint32_t mb = __float_as_uint(x.m), vb = __float_as_uint(x.v);
  const bool still = gate && mb == 0u && vb < 0x7f800000u;
  x.live = untouched && !still;
  x.idle = untouched && still && vb != 0u;
}
// One zero-gradient ApplyAdam update of two elements -- adam_dense1(g = 0) operation by operation -- with the packed square
// root / division.  The moments' updates are the IEEE operations themselves (v_pk_mul_f32 / v_pk_add_f32); what the guard
// has to cover is the operands of the square root and the division, and adam_win_guard1's bounds cover them for THIS formula
// too: with fast_ok (b1 in [0.85, 1), b2 in [0.5, 1)) 1 - b is exact, m1 = m - fl(m omb1) and v1 = v - fl(v omb2) are m b1 and
// v b2 to within 2 ulp and never larger in magnitude than m, v -- against a factor 4 of room between the guard's bounds
// (|n_j| >= 2^-92, v_j >= 2^-94) and the fast forms' domains (2^-94, 2^-96), and a factor 0.272 / 0.25 in b1^8 >= 1 / 4.  (The
// guard's v == +0 case needs m == +0: such an element is void here and never live.)
__device__ __forceinline__ void adam_zero_grad2_dense(rsx_f2& var, rsx_f2& m, rsx_f2& v, const float alpha, const float omb1,
                                                      const float omb2, const float eps) {
  m = m + (0.f - m) * omb1;
  v = v + (0.f - v) * omb2;
  const rsx_f2 n = m * alpha;
  const rsx_f2 d = rsx_sqrt2_fast(v) + eps;
  var = var - rsx_div2_fast(n, d);
}
// idle elements: v alone; live ones: update by update, each behind its own guard (adam_zero_grad1)
template <int NW, int N>
__device__ __forceinline__ void win_vec_update(WinVecEl (&x)[N], const Hp& h, const AlphaW& aw, const bool with_live = true) {
  bool any_idle = false, any_live = false;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    any_idle |= x[i].idle;
    any_live |= x[i].live;
  }
  if (__builtin_amdgcn_ballot_w64(any_idle) != 0ull) {          // (wave-uniform)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float v = x[i].v;
#pragma unroll
      for (int j = 0; j < 1 + NW; ++j) v = v + (0.f - v) * h.omb2;      // adam_dense1's v1 with g * g = +0
      if (x[i].idle) x[i].v = v;
    }
  }
  if (with_live && __builtin_amdgcn_ballot_w64(any_live) != 0ull) {
    // a wave with a live element outside the packed form's guard (or hyper-parameters outside): update by update, each behind its own guard
#pragma unroll 1
    for (int j = 0; j < 1 + NW; ++j) {
      Hp hj = h;
      if (j > 0) hj.alpha = aw.get(j - 1);
#pragma unroll
      for (int i = 0; i < N; ++i) adam_zero_grad1<true>(x[i].var, x[i].m, x[i].v, x[i].live, hj);
    }
  }
}
template <int NW>
__device__ __forceinline__ void adam_window_vec_block(const AdamArgs& a, const SegDev& s, const uint32_t blk, const int tid) {
  static_assert(ADAM_U_WVEC == 2, "two float4 per lane, both in flight at once");
  // the segment's fields, once (DESIGN 4c rule 6: `s` is a dynamically indexed kernel argument, every use is a load)
  float* const __restrict__ var1 = s.var;
  float* const __restrict__ m1 = s.m;
  float* const __restrict__ v1 = s.v;
  const int32_t* const __restrict__ slot = s.slot;
  const long long n = s.n;
  const long long base = (long long)(blk - s.blk_begin) * ADAM_Q_WVEC;
  const int32_t* const __restrict__ swb = a.slot_w0;
  const long long sws = a.slot_w_stride;
  Hp h;
  h.b1 = a.b1;
  h.b2 = a.b2;
  h.omb1 = 1.0f - a.b1;
  h.omb2 = 1.0f - a.b2;
  h.eps = a.eps;
  AlphaW aw;
  adam_step_sizes(a, NW, h.alpha, aw);
  const bool gate = win_shortcut_gate<NW>(a, h.alpha, aw) && __float_as_uint(h.omb1) < 0x7f800000u &&
                    __float_as_uint(h.omb2) < 0x7f800000u;
  bool fast_ok;
  const uint32_t m_lo_bits = win_fast_form<NW>(a, h.alpha, aw, fast_ok);
  const long long n4 = n >> 2;
  if (n4 > 0) {
    float4* const __restrict__ var4 = reinterpret_cast<float4*>(var1);
    float4* const __restrict__ m4 = reinterpret_cast<float4*>(m1);
    float4* const __restrict__ v4 = reinterpret_cast<float4*>(v1);
    const long long e0 = base + tid, e1 = e0 + ADAM_T;
    const bool in0 = e0 < n4, in1 = e1 < n4;
    const long long c0 = in0 ? e0 : n4 - 1, c1 = in1 ? e1 : n4 - 1;
    int4 t0 = reinterpret_cast<const int4*>(slot)[c0], t1 = reinterpret_cast<const int4*>(slot)[c1];
    // (untouched = -1 = all ones: one value >= 0 clears the sign of the AND.)  All of them in flight at once.
#pragma unroll
    for (int l = 0; l < NW; ++l) {
      const int4* const w = reinterpret_cast<const int4*>(swb + (long long)l * sws);
      const int4 w0 = w[c0], w1 = w[c1];
      t0.x &= w0.x; t0.y &= w0.y; t0.z &= w0.z; t0.w &= w0.w;
      t1.x &= w1.x; t1.y &= w1.y; t1.z &= w1.z; t1.w &= w1.w;
    }
    const float4 mm0 = m4[c0], vv0 = v4[c0], va0 = var4[c0], mm1 = m4[c1], vv1 = v4[c1], va1 = var4[c1];
    WinVecEl x[8] = {{va0.x, mm0.x, vv0.x, false, false}, {va0.y, mm0.y, vv0.y, false, false},
                     {va0.z, mm0.z, vv0.z, false, false}, {va0.w, mm0.w, vv0.w, false, false},
                     {va1.x, mm1.x, vv1.x, false, false}, {va1.y, mm1.y, vv1.y, false, false},
                     {va1.z, mm1.z, vv1.z, false, false}, {va1.w, mm1.w, vv1.w, false, false}};
    win_vec_classify(x[0], in0 && t0.x < 0, gate);
    win_vec_classify(x[1], in0 && t0.y < 0, gate);
    win_vec_classify(x[2], in0 && t0.z < 0, gate);
    win_vec_classify(x[3], in0 && t0.w < 0, gate);
    win_vec_classify(x[4], in1 && t1.x < 0, gate);
    win_vec_classify(x[5], in1 && t1.y < 0, gate);
    win_vec_classify(x[6], in1 && t1.z < 0, gate);
    win_vec_classify(x[7], in1 && t1.w < 0, gate);
    // every live element of the wave inside adam_win_guard1 (evaluated once, on the loaded state; fast_ok / m_lo_bits:
    // win_fast_form): the packed chain, two elements per instruction -- what it computes in the other elements is dropped.
    // (Named pairs: an array of them indexed inside the step loop is demoted to LDS by this toolchain.)
#define RSX_WV_BAD(i) (x[i].live && adam_win_guard1(x[i].var, x[i].m, x[i].v, m_lo_bits))
    const bool bad = !fast_ok | RSX_WV_BAD(0) | RSX_WV_BAD(1) | RSX_WV_BAD(2) | RSX_WV_BAD(3) | RSX_WV_BAD(4) | RSX_WV_BAD(5) |
                     RSX_WV_BAD(6) | RSX_WV_BAD(7);
#undef RSX_WV_BAD
    const bool packed = __builtin_amdgcn_ballot_w64(bad) == 0ull;      // (wave-uniform)
    const bool any_live = x[0].live | x[1].live | x[2].live | x[3].live | x[4].live | x[5].live | x[6].live | x[7].live;
    win_vec_update<NW>(x, h, aw, !packed);
    if (packed && __builtin_amdgcn_ballot_w64(any_live) != 0ull) {
      rsx_f2 va01 = {x[0].var, x[1].var}, va23 = {x[2].var, x[3].var}, va45 = {x[4].var, x[5].var}, va67 = {x[6].var, x[7].var};
      rsx_f2 mm01 = {x[0].m, x[1].m}, mm23 = {x[2].m, x[3].m}, mm45 = {x[4].m, x[5].m}, mm67 = {x[6].m, x[7].m};
      rsx_f2 vv01 = {x[0].v, x[1].v}, vv23 = {x[2].v, x[3].v}, vv45 = {x[4].v, x[5].v}, vv67 = {x[6].v, x[7].v};
      const float omb1 = h.omb1, omb2 = h.omb2, eps = h.eps;      // (scalars: `h` by reference here sent it to LDS)
      auto step = [&](const float alpha) {
        adam_zero_grad2_dense(va01, mm01, vv01, alpha, omb1, omb2, eps);
        adam_zero_grad2_dense(va23, mm23, vv23, alpha, omb1, omb2, eps);
        adam_zero_grad2_dense(va45, mm45, vv45, alpha, omb1, omb2, eps);
        adam_zero_grad2_dense(va67, mm67, vv67, alpha, omb1, omb2, eps);
      };
      step(h.alpha);
#pragma unroll 1
      for (int j = 0; j < NW; ++j) step(aw.get(j));
#define RSX_WV_TAKE(i, VA, MM, VV, c) if (x[i].live) { x[i].var = VA.c; x[i].m = MM.c; x[i].v = VV.c; }
      RSX_WV_TAKE(0, va01, mm01, vv01, x) RSX_WV_TAKE(1, va01, mm01, vv01, y)
      RSX_WV_TAKE(2, va23, mm23, vv23, x) RSX_WV_TAKE(3, va23, mm23, vv23, y)
      RSX_WV_TAKE(4, va45, mm45, vv45, x) RSX_WV_TAKE(5, va45, mm45, vv45, y)
      RSX_WV_TAKE(6, va67, mm67, vv67, x) RSX_WV_TAKE(7, va67, mm67, vv67, y)
#undef RSX_WV_TAKE
    }
    const bool live0 = x[0].live | x[1].live | x[2].live | x[3].live, live1 = x[4].live | x[5].live | x[6].live | x[7].live;
    const bool idle0 = x[0].idle | x[1].idle | x[2].idle | x[3].idle, idle1 = x[4].idle | x[5].idle | x[6].idle | x[7].idle;
    if (live0) {
      var4[c0] = make_float4(x[0].var, x[1].var, x[2].var, x[3].var);
      m4[c0] = make_float4(x[0].m, x[1].m, x[2].m, x[3].m);
    }
    if (live0 || idle0) v4[c0] = make_float4(x[0].v, x[1].v, x[2].v, x[3].v);
    if (live1) {
      var4[c1] = make_float4(x[4].var, x[5].var, x[6].var, x[7].var);
      m4[c1] = make_float4(x[4].m, x[5].m, x[6].m, x[7].m);
    }
    if (live1 || idle1) v4[c1] = make_float4(x[4].v, x[5].v, x[6].v, x[7].v);
  }
  // scalar tail (n not a multiple of 4): the wave that holds float4 position n4's lane -- the block the layout adds for it
  // (work = n / 4 + 1) -- takes the 1 .. 3 last elements in lanes 0 .. 2, maps hoisted the same way
  const int nt = (int)(n & 3);
  const long long tp = n4 - base;                                 // position n4 within this block
  if (nt != 0 && tp >= 0 && tp < ADAM_Q_WVEC && (tid >> 6) == (int)((tp & (ADAM_T - 1)) >> 6)) {      // (wave-uniform)
    const int q = tid & 63;
    const bool mine = q < nt;
    const long long i = n4 * 4 + (mine ? q : 0);
    int t = slot[i];
#pragma unroll
    for (int l = 0; l < NW; ++l) t &= swb[(long long)l * sws + i];
    WinVecEl x = {var1[i], m1[i], v1[i], false, false};
    win_vec_classify(x, mine && t < 0, gate);
    if (__builtin_amdgcn_ballot_w64(x.idle) != 0ull) {
      float v = x.v;
#pragma unroll
      for (int j = 0; j < 1 + NW; ++j) v = v + (0.f - v) * h.omb2;
      if (x.idle) x.v = v;
    }
    if (__builtin_amdgcn_ballot_w64(x.live) != 0ull) {
#pragma unroll 1
      for (int j = 0; j < 1 + NW; ++j) {
        Hp hj = h;
        if (j > 0) hj.alpha = aw.get(j - 1);
        adam_zero_grad1<true>(x.var, x.m, x.v, x.live, hj);
      }
    }
    if (x.live) {
      var1[i] = x.var;
      m1[i] = x.m;
    }
    if (x.live || x.idle) v1[i] = x.v;
  }
}

template <int NW, int U = ADAM_U, bool COMPACT = false>
__device__ __forceinline__ void adam_window_block(const AdamArgs& a, const uint32_t blk, const int tid = threadIdx.x,
                                                  uint32_t* const lds = nullptr /* COMPACT: WIN_LIST_WORDS words of LDS */) {
  constexpr int nw = NW;        // == a.nw (the host picks the instantiation)
  constexpr int HB = RSX_ADAM_WIN_HB;
  constexpr int NB = U / HB;
  static_assert(U % HB == 0 && U <= ADAM_U, "U");
  static_assert(!COMPACT || (U == ADAM_U && ADAM_T % 64 == 0), "the compact form: full-size blocks of whole waves");
  int si = 0;
#pragma unroll 1
  for (int k = 1; k < a.nseg; ++k)
    if (blk >= a.seg[k].blk_begin) si = k;
  const SegDev& s = a.seg[si];
  if (s.kind != RSX_ADAM_TABLE_TF1_COLD) {
    if constexpr (U == ADAM_U) {         // the stand-alone launch (a.win_u == 0): the vector's blocks are ADAM_U_WVEC wide
      if (s.kind == RSX_ADAM_VEC_COLD) {
        adam_window_vec_block<NW>(a, s, blk, tid);
        return;
      }
    }
    adam_block(a, blk, tid);
    return;
  }
  Hp h;
  h.b1 = a.b1;
  h.b2 = a.b2;
  h.omb1 = 1.0f - a.b1;
  h.omb2 = 1.0f - a.b2;
  h.eps = a.eps;
  AlphaW aw;
  adam_step_sizes(a, nw, h.alpha, aw);
  bool fast_ok;
  const uint32_t m_lo_bits = win_fast_form<NW>(a, h.alpha, aw, fast_ok);
  const int32_t* __restrict__ swb = a.slot_w0;
  const int sws = (int)a.slot_w_stride;           // (< 2^28: adam_build_args) 32-bit element offsets: scalar base + vector offset
  float4* __restrict__ var4 = reinterpret_cast<float4*>(s.var);
  float4* __restrict__ m4 = reinterpret_cast<float4*>(s.m);
  float4* __restrict__ v4 = reinterpret_cast<float4*>(s.v);
  const long long base = (long long)(blk - s.blk_begin) * ((long long)ADAM_T * U);
  const int lpr = s.d >> 2;
  const long long n4 = s.n * lpr;
  const bool pow2 = (lpr & (lpr - 1)) == 0;
  const int lsh = 31 - __clz(lpr);
  struct Batch {
    float4 var[HB], m[HB], v[HB];
    long long ec[HB];
    int t[HB];
    bool live[HB];
  };
  auto load_state = [&](Batch& B, const bool with_var) {
#pragma unroll
    for (int u = 0; u < HB; ++u) {
#if RSX_ADAM_NT
      if (with_var) B.var[u] = __builtin_nontemporal_load(&var4[B.ec[u]]);
      B.m[u] = __builtin_nontemporal_load(&m4[B.ec[u]]);
      B.v[u] = __builtin_nontemporal_load(&v4[B.ec[u]]);
#else
      if (with_var) B.var[u] = var4[B.ec[u]];
      B.m[u] = m4[B.ec[u]];
      B.v[u] = v4[B.ec[u]];
#endif
    }
  };
  auto issue = [&](const int b, Batch& B, const bool with_var = true) {
#pragma unroll
    for (int u = 0; u < HB; ++u) {
      const long long e = base + (long long)(b * HB + u) * ADAM_T + tid;
      B.ec[u] = e < n4 ? e : n4 - 1;
      B.live[u] = e < n4;
      const long long row = pow2 ? (B.ec[u] >> lsh) : (B.ec[u] / lpr);
      B.t[u] = s.slot[row];
      // (untouched = -1 = all ones: one value >= 0 clears the sign of the AND.)  All of them in flight at once.
#pragma unroll
      for (int l = 0; l < NW; ++l) B.t[u] &= swb[l * sws + (int)row];
    }
    load_state(B, with_var);
  };
  auto store = [&](const Batch& B) {
#pragma unroll
    for (int u = 0; u < HB; ++u) {
      if (B.live[u] && B.t[u] < 0) {
#if RSX_ADAM_NT
        __builtin_nontemporal_store(B.var[u], &var4[B.ec[u]]);
        __builtin_nontemporal_store(B.m[u], &m4[B.ec[u]]);
        __builtin_nontemporal_store(B.v[u], &v4[B.ec[u]]);
#else
        var4[B.ec[u]] = B.var[u];
        m4[B.ec[u]] = B.m[u];
        v4[B.ec[u]] = B.v[u];
#endif
      }
    }
  };
  // Batches in which some element of the wave leaves the packed forms' domain are left untouched by the pipeline and redone
  // in the IEEE form after it, from memory (a wave-uniform decision; the hot loop then holds the packed form only).
  // (bit b: batch b of the block; COMPACT, bit NB + b: batch b of the list)
  uint32_t redo = 0u;
  auto finish = [&](const int b, Batch& B) {
    bool bad = !fast_ok;
#pragma unroll
    for (int u = 0; u < HB; ++u) bad |= adam_win_guard4(B.var[u], B.m[u], B.v[u], m_lo_bits);
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull) {
      redo |= 1u << b;
      return;
    }
    rsx_f2 var2[HB][2], m2[HB][2], v2[HB][2];
#pragma unroll
    for (int u = 0; u < HB; ++u) {
      var2[u][0] = (rsx_f2){B.var[u].x, B.var[u].y}; var2[u][1] = (rsx_f2){B.var[u].z, B.var[u].w};
      m2[u][0] = (rsx_f2){B.m[u].x, B.m[u].y}; m2[u][1] = (rsx_f2){B.m[u].z, B.m[u].w};
      // (v == +0, which the guard admits under m == +0 only: compute with 1, store the zero back)
      v2[u][0] = (rsx_f2){B.v[u].x == 0.f ? 1.f : B.v[u].x, B.v[u].y == 0.f ? 1.f : B.v[u].y};
      v2[u][1] = (rsx_f2){B.v[u].z == 0.f ? 1.f : B.v[u].z, B.v[u].w == 0.f ? 1.f : B.v[u].w};
    }
    auto step = [&](const float alpha) {
#pragma unroll
      for (int u = 0; u < HB; ++u) {
        adam_zero_grad2(var2[u][0], m2[u][0], v2[u][0], alpha, h);
        adam_zero_grad2(var2[u][1], m2[u][1], v2[u][1], alpha, h);
      }
    };
    step(h.alpha);
#pragma unroll 1
    for (int j = 0; j < NW; ++j) step(aw.get(j));
#pragma unroll
    for (int u = 0; u < HB; ++u) {
      B.var[u] = make_float4(var2[u][0].x, var2[u][0].y, var2[u][1].x, var2[u][1].y);
      B.m[u] = make_float4(m2[u][0].x, m2[u][0].y, m2[u][1].x, m2[u][1].y);
      B.v[u] = make_float4(B.v[u].x == 0.f ? 0.f : v2[u][0].x, B.v[u].y == 0.f ? 0.f : v2[u][0].y,
                           B.v[u].z == 0.f ? 0.f : v2[u][1].x, B.v[u].w == 0.f ? 0.f : v2[u][1].y);
    }
    store(B);
  };
  // COMPACT, phase 2: batch b of the list is entries [b * ADAM_T * HB, ...), 64 * HB consecutive ones per wave; the wave that
  // takes the first ones rotates with the block (a short list keeps one wave busy: not the same SIMD's every time)
  const int lane = tid & 63;
  const uint32_t wave_first = (((uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6) + blk) % (ADAM_T / 64u)) * (64u * HB);
  uint32_t n_live = 0u;
  auto listed = [&](const int b) { return (uint32_t)b * (ADAM_T * HB) + wave_first < n_live; };      // (wave-uniform)
  auto issue_listed = [&](const int b, Batch& B) {
#pragma unroll
    for (int u = 0; u < HB; ++u) {
      const uint32_t idx = (uint32_t)b * (ADAM_T * HB) + wave_first + (uint32_t)u * 64u + (uint32_t)lane;
      B.live[u] = idx < n_live;
      B.ec[u] = base + (B.live[u] ? lds[idx] : 0u);      // (beyond the list: the block's first float4, loaded and dropped)
      B.t[u] = -1;
    }
    load_state(B, true);
  };
  if constexpr (COMPACT) {
    const bool gate = win_shortcut_gate<NW>(a, h.alpha, aw);
    const unsigned long long row_lanes = (lpr >= 64 ? ~0ull : (1ull << lpr) - 1ull) << (lane & ~(lpr - 1));
    uint32_t* const list_n = lds + ADAM_T * U;
    if (tid == 0) *list_n = 0u;
    __syncthreads();
    // the row's lanes vote: untouched (some update is due), still (void or idle: var and m keep their bits), row_v0 (void)
    auto vote = [&](const Batch& B, const int u, bool& untouched, bool& still, bool& row_v0) {
      const uint32_t mx = __float_as_uint(B.m[u].x), my = __float_as_uint(B.m[u].y), mz = __float_as_uint(B.m[u].z),
                     mw = __float_as_uint(B.m[u].w);
      const uint32_t vx = __float_as_uint(B.v[u].x), vy = __float_as_uint(B.v[u].y), vz = __float_as_uint(B.v[u].z),
                     vw = __float_as_uint(B.v[u].w);
      const uint32_t v_top = max(max(vx, vy), max(vz, vw));         // <= the bits of +inf: no sign, no NaN
      const bool row_m0 = (__builtin_amdgcn_ballot_w64((mx | my | mz | mw) != 0u) & row_lanes) == 0ull;
      const bool row_vok = (__builtin_amdgcn_ballot_w64(v_top > 0x7f800000u) & row_lanes) == 0ull;
      row_v0 = (__builtin_amdgcn_ballot_w64((vx | vy | vz | vw) != 0u) & row_lanes) == 0ull;
      untouched = B.live[u] && B.t[u] < 0;
      still = gate && row_m0 && row_vok;
    };
    // Is every row of this wave's first batch that has updates due a live one (and is there one)?  Then the wave takes the
    // one-pass pipeline for its share of the block (right for any rows): where the tables have filled up, the compact form
    // costs the one-pass form's time and a look at one batch
    auto wave_dense = [&](const Batch& B) {
      unsigned long long due = 0ull, spared = 0ull;
#pragma unroll
      for (int u = 0; u < HB; ++u) {
        bool untouched, still, row_v0;
        vote(B, u, untouched, still, row_v0);
        due |= __builtin_amdgcn_ballot_w64(untouched);
        spared |= __builtin_amdgcn_ballot_w64(untouched && still);
      }
      return !gate || (due != 0ull && spared == 0ull);
    };
    auto classify = [&](const Batch& B) {
      unsigned long long lm[HB];
      bool is_live[HB];
      uint32_t total = 0u;
#pragma unroll
      for (int u = 0; u < HB; ++u) {
        bool untouched, still, row_v0;
        vote(B, u, untouched, still, row_v0);
        is_live[u] = untouched && !still;
        lm[u] = __builtin_amdgcn_ballot_w64(is_live[u]);
        total += (uint32_t)__popcll(lm[u]);
        if (untouched && still && !row_v0) {                        // idle: v alone moves
          float4 v = B.v[u];
#pragma unroll
          for (int j = 0; j < 1 + NW; ++j) {
            v.x = v.x * h.b2;
            v.y = v.y * h.b2;
            v.z = v.z * h.b2;
            v.w = v.w * h.b2;
          }
#if RSX_ADAM_NT
          __builtin_nontemporal_store(v, &v4[B.ec[u]]);
#else
          v4[B.ec[u]] = v;
#endif
        }
      }
      if (total != 0u) {                                            // (wave-uniform)
        uint32_t at = 0u;
        if (lane == 0) at = atomicAdd(list_n, total);
        at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
#pragma unroll
        for (int u = 0; u < HB; ++u) {
          const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(lm[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lm[u], 0u));
          if (is_live[u]) lds[at + before] = (uint32_t)(B.ec[u] - base);
          at += (uint32_t)__popcll(lm[u]);
        }
      }
    };
    bool dense;
    {
      Batch bt[2];
      issue(0, bt[0], false);
      dense = wave_dense(bt[0]);                                    // (wave-uniform)
      if (!dense) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (b + 1 < NB) issue(b + 1, bt[(b + 1) & 1], false);
          classify(bt[b & 1]);
        }
      }
    }
    __syncthreads();
    n_live = (uint32_t)__builtin_amdgcn_readfirstlane((int)*list_n);
    {
      Batch bt[2];
      if (listed(0)) issue_listed(0, bt[0]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b + 1 < NB && listed(b + 1)) issue_listed(b + 1, bt[(b + 1) & 1]);
        if (listed(b)) finish(NB + b, bt[b & 1]);
      }
    }
    // (after the list, not before the barrier: the other waves do not wait for it, and with the two pipelines' live ranges
    // apart the kernel needs no scratch)
    if (dense) {                                                    // the one-pass form's pipeline for this wave's lanes
      Batch bt[2];
      issue(0, bt[0]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b + 1 < NB) issue(b + 1, bt[(b + 1) & 1]);
        finish(b, bt[b & 1]);
      }
    }
  } else {
    Batch bt[2];
    issue(0, bt[0]);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b + 1 < NB) issue(b + 1, bt[(b + 1) & 1]);
      finish(b, bt[b & 1]);
    }
  }
  redo = __builtin_amdgcn_readfirstlane(redo);
  if (redo != 0u) {
#pragma unroll 1
    for (int b = 0; b < (COMPACT ? 2 * NB : NB); ++b) {
      if (!(redo >> b & 1u)) continue;
      Batch B;
      if (COMPACT && b >= NB) issue_listed(b - NB, B);
      else issue(b, B);
#pragma unroll
      for (int u = 0; u < HB; ++u) {     // (unrolled: a dynamically indexed register array is demoted to scratch)
        F4_APPLY(adam_sparse1, B.var[u], B.m[u], B.v[u], F4Z, false, h);
#pragma unroll 1
        for (int j = 0; j < NW; ++j) {          // the later steps of the window, back to back in registers
          Hp hj = h;
          hj.alpha = aw.get(j);
          F4_APPLY(adam_sparse1, B.var[u], B.m[u], B.v[u], F4Z, false, hj);
        }
      }
      store(B);
    }
  }
}

// Host: validates the segment list and lays the segments out over the launch-wide block index space.
// Returns an rsx_status; *blocks_out = number of workgroups (0 when there is nothing to do).
static inline int adam_build_args(const rsx_adam_seg* segs_h, int nseg, float* state, float lr, float beta1, float beta2,
                                  float eps, AdamArgs& a, uint32_t* blocks_out, int win_u = 0, int alpha_src = 0) {
  if (!segs_h || !state || nseg <= 0 || nseg > RSX_ADAM_MAX_SEGS) return RSX_EINVAL;
  if (win_u != 0 && win_u != 2 && win_u != 4 && win_u != ADAM_U) return RSX_EINVAL;
  a.win_u = win_u == ADAM_U ? 0 : win_u;
  a.alpha_src = alpha_src ? 1 : 0;
  uint32_t blocks = 0;
  int k = 0, n_cold = 0;
  a.nw = 0;
  a.slot_w0 = nullptr;
  a.slot_w_stride = 0;
  for (int i = 0; i < nseg; ++i) {
    const rsx_adam_seg& s = segs_h[i];
    if (s.n < 0 || !s.var || !s.m || !s.v) return RSX_EINVAL;
    long long work;  // float4 (or slot) units
    switch (s.kind) {
      case RSX_ADAM_DENSE:
        if (!s.g) return RSX_EINVAL;
        if (s.B > 1 && (s.stride < s.n || (s.stride & 3))) return RSX_EINVAL;     // replica sum: 16-byte aligned blocks
        work = (s.n >> 2) + 1;
        break;
      case RSX_ADAM_TABLE_TF1:
      case RSX_ADAM_TABLE_TF1_COLD:
        if (!s.slot || (!s.g && s.kind == RSX_ADAM_TABLE_TF1) || s.d < 4 || (s.d & 3)) return RSX_EINVAL;
        if (s.kind == RSX_ADAM_TABLE_TF1 && s.slot_w[0]) return RSX_EINVAL;          // windows: COLD kinds only
        work = s.n * (s.d >> 2);
        break;
      case RSX_ADAM_VEC_SLOT:
      case RSX_ADAM_VEC_COLD:
        if (!s.slot || (!s.g && s.kind == RSX_ADAM_VEC_SLOT)) return RSX_EINVAL;
        if (s.kind == RSX_ADAM_VEC_SLOT && s.slot_w[0]) return RSX_EINVAL;
        work = (s.n >> 2) + 1;
        break;
      case RSX_ADAM_TABLE_ROWS:
        if (!s.g || !s.uniq_row || !s.nuniq || s.B <= 0 || s.d < 4 || (s.d & 3)) return RSX_EINVAL;
        if (s.g_replicas > 1 && (s.g_replica_stride <= 0 || (s.g_replica_stride & 3) || s.g_replica_stride >= (1ll << 33))) return RSX_EINVAL;
        work = s.n * (s.d >> 2);
        break;
      case RSX_ADAM_VEC_ROWS:
      case RSX_ADAM_VEC_ROWS_DENSE:
        if (!s.g || !s.uniq_row || !s.nuniq || s.B <= 0) return RSX_EINVAL;
        if (s.g_replicas > 1 && (s.g_replica_stride <= 0 || (s.g_replica_stride & 3) || s.g_replica_stride >= (1ll << 33))) return RSX_EINVAL;
        work = s.n;
        break;
      default: return RSX_EINVAL;
    }
    if (s.n == 0) continue;
    SegDev& d = a.seg[k++];
    d.kind = s.kind;
    d.d = s.d;
    d.n = s.n;
    d.var = s.var;
    d.m = s.m;
    d.v = s.v;
    d.g = s.g;
    d.slot = s.slot;
    d.uniq_row = s.uniq_row;
    d.nuniq = s.nuniq;
    d.B = s.B;
    d.stride = s.stride;
    d.zero_grad = s.zero_grad;
    const bool rows_kind = s.kind == RSX_ADAM_TABLE_ROWS || s.kind == RSX_ADAM_VEC_ROWS || s.kind == RSX_ADAM_VEC_ROWS_DENSE;
    d.g_rep = rows_kind && s.g_replicas > 1 ? s.g_replicas : 1;
    d.g_rep_stride4 = d.g_rep > 1 ? (int32_t)(s.g_replica_stride >> 2) : 0;
    if (s.kind == RSX_ADAM_TABLE_TF1_COLD || s.kind == RSX_ADAM_VEC_COLD) {     // the window's extra slot maps (AdamArgs)
      int nw = 0;
      while (nw < ADAM_WMAX && s.slot_w[nw] != nullptr) ++nw;
      for (int j = nw; j < ADAM_WMAX; ++j)
        if (s.slot_w[j] != nullptr) return RSX_EINVAL;                          // a prefix, no holes
      const long long str = nw > 1 ? (long long)(s.slot_w[1] - s.slot_w[0]) : 0;
      for (int j = 1; j < nw; ++j)
        if (s.slot_w[j] != s.slot_w[0] + j * str) return RSX_EINVAL;           // equally spaced (see rsx.h)
      if (nw > 0 && (reinterpret_cast<uintptr_t>(s.slot_w[0]) & 15u || (str & 3) || str < 0 || str >= (1ll << 28)))
        return RSX_EINVAL;                                                      // int4 reads (VEC_COLD), 32-bit offsets
      if (n_cold++ == 0) {
        a.nw = nw;
        a.slot_w0 = s.slot_w[0];
        a.slot_w_stride = str;
      } else if (nw != a.nw || (nw > 0 && (a.slot_w0 != s.slot_w[0] || a.slot_w_stride != str))) {
        return RSX_EINVAL;                                                      // one window per launch
      }
    }
    d.blk_begin = blocks;
    const long long quantum = s.kind == RSX_ADAM_DENSE ? ADAM_Q_DENSE
                              : (s.kind == RSX_ADAM_TABLE_TF1_COLD && a.win_u > 0 ? (long long)ADAM_T * a.win_u
                                 : (long long)ADAM_T * adam_vec_u(s.kind, a.nw, a.win_u));
    blocks += (uint32_t)((work + quantum - 1) / quantum);
  }
  a.nseg = k;
  a.lr = lr;
  a.b1 = beta1;
  a.b2 = beta2;
  a.eps = eps;
  a.state = state;
  a.total_blocks = blocks;
  *blocks_out = k == 0 ? 0u : blocks;
  return RSX_OK;
}

// A slice [blk_lo, blk_hi) of a COLD sweep carried by another kernel's launch as extra workgroups.
struct AdamSlice {
  AdamArgs args;
  uint32_t blk_lo, n_blk;     // n_blk == 0: no slice
};
// Workgroup order of a carrier launch with T workgroups of its own and R riders.  Appending the riders after the carrier's
// workgroups serialises the two when T alone fills the chip (every slot is taken by a latency/MFMA-bound tile until the
// first ones retire; the HBM-bound riders then run alone: measured, cin_bwd_dw_bf16_k 35 us + 27 us = 62 us).  Dealing them
// in alternating runs of 8 (consecutive workgroup ids go to the 8 XCDs round-robin, so both kinds land on every XCD) makes
// both resident from the start.  -> rider? and the index within its kind.
struct RiderSplit {
  bool rider;
  uint32_t idx;
};
__device__ __forceinline__ RiderSplit rider_split(const uint32_t lin, const uint32_t T, const uint32_t R) {
  const uint32_t m8 = (T < R ? T : R) & ~7u;          // alternating part: m8 of each kind
  if (lin < 2u * m8) return {(lin & 8u) != 0u, ((lin >> 4) << 3) | (lin & 7u)};
  const uint32_t r = lin - 2u * m8;                   // the rest: the carrier's own first
  if (r < T - m8) return {false, m8 + r};
  return {true, m8 + (r - (T - m8))};
}

static inline int adam_build_slice(const rsx_adam_slice* sl_h, AdamSlice& out) {
  out.n_blk = 0;
  out.blk_lo = 0;
  if (sl_h == nullptr) return RSX_OK;
  uint32_t blocks = 0;
  const int rc = adam_build_args(sl_h->segs, sl_h->nseg, sl_h->state, sl_h->lr, sl_h->beta1, sl_h->beta2, sl_h->eps,
                                 out.args, &blocks, sl_h->window_block_u, sl_h->alphas_from_state);
  if (rc != RSX_OK) return rc;
  if (sl_h->blk_hi < sl_h->blk_lo || sl_h->blk_hi > blocks) return RSX_EINVAL;
  out.blk_lo = sl_h->blk_lo;
  out.n_blk = sl_h->blk_hi - sl_h->blk_lo;
  return RSX_OK;
}
