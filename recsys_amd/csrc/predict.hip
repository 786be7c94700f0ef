// Serving forward of fm.py / deepfm.py as ONE launch: ids [B, F] -> prob [B] (include/rsx.h rsx_predict_fm_tower).
// Reference: deepfm/deepfm.py:85-113 in PREDICT mode (input_layer lookup, first-order one-hot matmul, FM term,
// L x [dense(relu) -> batch_normalization(training=False) -> dropout(training=False)], the 1-unit layer, the 3 -> 1 logits
// layer, sigmoid) and fm/fm.py:117-134 (the same without the tower: L = 0, two head inputs).
//
// In inference form nothing crosses the rows of a batch: the reference never updates the moving statistics, so batch-norm is
// the per-element affine gamma * x / sqrt(1 + eps) + beta, and dropout is the identity.  A workgroup therefore owns a tile of
// 16 examples from the ids to the probability: their F rows are gathered straight into LDS (the first layer's MFMA A operand,
// as tower_gather_fwd_k does), first-order sum and FM term are formed from the same registers, every layer's 16 x N activation
// tile stays in LDS, and only prob is written.  No E / S / statistics / gradient-side outputs, no workspace, no atomics: a row's
// bits depend on its own ids and the weights only (not on its position in the tile, nor on the rest of the batch).
//
// Weights are streamed from L2 (W0 of deepfm.py is 624 x 100 fp32 = 250 KB, more than the 160 KB of LDS).  A lone wave issues
// only ~270 instructions per microsecond, so the layer loop is shaped by instructions per MFMA, not by bytes: a wave owns a
// GROUP of 64 columns = 4 MFMA tiles whose lane i holds columns 4 i .. 4 i + 3, so that ONE 16-byte load per k feeds the B
// operands of 4 MFMAs (tile t takes column 4 i + t), and one 16-byte LDS read per k-step feeds the A operands of 16.  The first
// form of this kernel (a 16-column tile per wave, one 4-byte load per MFMA) took 30 us per launch whatever the batch; see
// DESIGN.md.  K is split over the waves a layer's groups leave free (100 columns = 2 groups -> 4 K-splits); the partial tiles
// meet in LDS and are added in split order by the epilogue (bias, relu, the batch-norm affine).
// MFMA: v_mfma_f32_16x16x4_f32, an exact-fp32 chain.  Lane (i = lane & 15, kq = lane >> 4): A operand row i, B operand column
// of lane i, k = 16 ks + 4 kq + t over the four MFMAs t of k-step ks (tower.hip's convention); the accumulator holds rows
// 4 kq + r.  The 4 tiles of a group are 4 independent chains (a dependent 16x16x4 fp32 MFMA waits ~32 cycles).
#include "rsx_common.h"

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int PR_T = 512, PR_NW = PR_T / 64;   // threads / waves per workgroup
constexpr int PR_ROWS = 16;                    // examples per workgroup
constexpr int PR_GF = 8;                       // fields per gather thread: 64 fields / 8 field lanes
constexpr int PR_MAX_LDS = 160 * 1024;

struct PredictArgs {
  const float* tables; const float* w1; const int32_t* row_off; const int32_t* ids;
  const float* W[RSX_PREDICT_MAX_LAYERS]; const float* b[RSX_PREDICT_MAX_LAYERS];
  const float* gamma[RSX_PREDICT_MAX_LAYERS]; const float* beta[RSX_PREDICT_MAX_LAYERS];
  const float* wd; const float* bd; const float* c0; const float* wo; const float* bo;
  float* prob;
  uint64_t w1_mask;
  float bn_rstd;                               // 1 / sqrt(1 + eps)
  int B, F, L;
  int N[RSX_PREDICT_MAX_LAYERS];
  int ksplit[RSX_PREDICT_MAX_LAYERS];          // K-splits of a layer: its column groups x ksplit work units go round the 8 waves
  int ldx, lda;                                // row strides of the gathered tile and of the activation tiles (floats, == 4 mod 8)
  int oA0, oA1, oP, oY;                        // LDS offsets (floats): activation tiles, partial tiles, y1 | y2 [2][16]
};

// B operands of one k-step for a column group: b[t] = W[16 ks + 4 kq + t][c0 .. c0 + 3].  Rows past K are clamped to K - 1 (the A
// operand is zero there), columns past N to a valid address (their outputs are dropped).  VEC: N % 4 == 0 and W 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ void load_b(f32x4 (&b)[4], const float* __restrict__ W, const int ks, const int K, const uint32_t N,
                                       const int kq, const uint32_t c0) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = 16 * ks + 4 * kq + t;
    const uint32_t o = (uint32_t)(k < K ? k : K - 1) * N;
    if (VEC) {
      b[t] = *reinterpret_cast<const f32x4*>(W + (o + c0));
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) b[t][c] = W[o + (c0 + c < N ? c0 + c : N - 1)];
    }
  }
}

__device__ __forceinline__ void mfma_step(f32x4 (&acc)[4], const float4 a, const f32x4 (&b)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mfma16(a.x, b[0][t], acc[t]);
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mfma16(a.y, b[1][t], acc[t]);
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mfma16(a.z, b[2][t], acc[t]);
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mfma16(a.w, b[3][t], acc[t]);
}

// part [ksplit][16][PW] <- the partial products in [16][ldi] . W [K][N] of this wave's (column group, K-split) units.  The B
// operands run one k-step ahead of the MFMAs (deeper prefetch and loading a layer's first operands ahead of the work that
// produces its input were measured and changed nothing or lost 1-2 us to their extra instructions: DESIGN.md).
template <bool VEC>
__device__ __forceinline__ void layer_mfma(const float* __restrict__ in, const int ldi, const int K, const float* __restrict__ W,
                                           const int N, const int ksplit, float* __restrict__ part, const int w, const int lane) {
  const int i = lane & 15, kq = lane >> 4;
  const int nks = (K + 15) >> 4, ng = (N + 63) >> 6, PW = ng * 64;
  const float* arow = in + i * ldi + 4 * kq;
  for (int u = w; u < ng * ksplit; u += PR_NW) {          // (wave-uniform)
    const int g = u % ng, sp = u / ng;
    const int ks_lo = sp * nks / ksplit, ks_hi = (sp + 1) * nks / ksplit;
    const uint32_t col = (uint32_t)(g * 64 + 4 * i);
    const uint32_t c0 = col < (uint32_t)N ? col : 0u;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 bc[4], bn[4];
    if (ks_lo < ks_hi) load_b<VEC>(bc, W, ks_lo, K, (uint32_t)N, kq, c0);
    for (int ks = ks_lo; ks < ks_hi; ++ks) {
      const bool more = ks + 1 < ks_hi;
      if (more) load_b<VEC>(bn, W, ks + 1, K, (uint32_t)N, kq, c0);      // (in flight under this k-step's 16 MFMAs)
      const float4 a = *reinterpret_cast<const float4*>(arow + 16 * ks);
      mfma_step(acc, a, bc);
      if (more) {
#pragma unroll
        for (int t = 0; t < 4; ++t) bc[t] = bn[t];
      }
    }
    float* pr = part + (sp * 16 + 4 * kq) * PW + g * 64 + 4 * i;
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(pr + r * PW) = f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
  }
}

// out [16][ldo] = gamma' * relu(sum of the partial tiles in split order + bias) + beta; the columns N .. up16(N) become zeros
// (the next layer's last k-step reads them).  Thread = (row, float4 column).
__device__ __forceinline__ void layer_epilogue(const float* __restrict__ part, const int ksplit, const int N,
                                               const float* __restrict__ bias, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, const float rstd, float* __restrict__ out,
                                               const int ldo, const int tid) {
  const int PW = ((N + 63) >> 6) * 64, NP = (N + 15) & ~15;
  const int row = tid >> 5;
  for (int c = 4 * (tid & 31); c < NP; c += 128) {
    f32x4 v = *reinterpret_cast<const f32x4*>(part + row * PW + c);
    for (int sp = 1; sp < ksplit; ++sp) v += *reinterpret_cast<const f32x4*>(part + (sp * 16 + row) * PW + c);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = c + e, cc = col < N ? col : N - 1;
      const float a = fmaxf(v[e] + bias[cc], 0.f);
      const float inv = gamma != nullptr ? rstd * gamma[cc] : 1.f;     // oracle / TF order: (rstd * gamma) * x + beta
      const float sh = beta != nullptr ? beta[cc] : 0.f;
      o[e] = col < N ? a * inv + sh : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + row * ldo + c) = o;
  }
}

__device__ __forceinline__ void dense_bn_layer(const float* in, const int ldi, const int K, const float* W, const float* bias,
                                               const float* gamma, const float* beta, const float rstd, const int N,
                                               const int ksplit, float* part, float* out, const int ldo, const int tid) {
  const int w = tid >> 6, lane = tid & 63;
  if ((N & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15u) == 0) layer_mfma<true>(in, ldi, K, W, N, ksplit, part, w, lane);
  else layer_mfma<false>(in, ldi, K, W, N, ksplit, part, w, lane);
  __syncthreads();
  layer_epilogue(part, ksplit, N, bias, gamma, beta, rstd, out, ldo, tid);
  __syncthreads();
}

__global__ __launch_bounds__(PR_T) void predict_fm_tower_k(const PredictArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS;
  const int F = p.F, ldx = p.ldx;
  float* X = lds;                                        // [16][ldx]: the examples' rows, field-major (= E.reshape(B, F * 16))
  float* ys = lds + p.oY;                                // y1 [16] | y2 [16]
  // ---- gather + first-order sum + FM term (the lane mapping of gather_device.h on half a wave per example): thread =
  // (example r, field lane j, float4 quarter q), fields j, j + 8, ...; ids and offsets first, then every row load, then the
  // stores and sums in ascending f.  Rows past the batch take the last example's ids (never ids past B); their outputs are
  // not stored. ----
  {
    const int r = tid >> 5, j = (tid >> 2) & 7, q = tid & 3;
    const f32x4* __restrict__ TV = reinterpret_cast<const f32x4*>(p.tables);
    const int b = row0 + r < p.B ? row0 + r : p.B - 1;
    const uint32_t ib = (uint32_t)b * (uint32_t)F;
    int row[PR_GF], fc[PR_GF];
#pragma unroll
    for (int u = 0; u < PR_GF; ++u) {
      const int f = j + 8 * u;
      fc[u] = f < F ? f : F - 1;
      row[u] = p.row_off[fc[u]] + p.ids[ib + (uint32_t)fc[u]];
    }
    f32x4 ev[PR_GF];
    float wv[PR_GF];
#pragma unroll
    for (int u = 0; u < PR_GF; ++u) {
      ev[u] = TV[(size_t)row[u] * 4 + q];
      wv[u] = p.w1 != nullptr ? p.w1[row[u]] : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);                   // (every load in flight before the first store)
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, qq = {0.f, 0.f, 0.f, 0.f};
    float a1 = 0.f;
#pragma unroll
    for (int u = 0; u < PR_GF; ++u) {
      if (j + 8 * u < F) {
        *reinterpret_cast<f32x4*>(X + r * ldx + fc[u] * 16 + q * 4) = ev[u];
        s += ev[u];
        qq += ev[u] * ev[u];
        if ((p.w1_mask >> fc[u]) & 1ull) a1 += wv[u];
      }
    }
#pragma unroll
    for (int m = 4; m < 32; m <<= 1) {                   // over the field lanes j
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[e] += __shfl_xor(s[e], m);
        qq[e] += __shfl_xor(qq[e], m);
      }
      a1 += __shfl_xor(a1, m);
    }
    float t = ((s[0] * s[0] - qq[0]) + (s[1] * s[1] - qq[1])) + ((s[2] * s[2] - qq[2]) + (s[3] * s[3] - qq[3]));
    t += __shfl_xor(t, 1);                               // over the quarters q
    t += __shfl_xor(t, 2);
    if ((tid & 31) == 0) {
      ys[r] = a1;
      ys[16 + r] = 0.5f * t;
    }
  }
  __syncthreads();
  // ---- the tower: activation tiles ping-pong between two LDS buffers ----
  float* A0 = lds + p.oA0;
  float* A1 = lds + p.oA1;
  float* part = lds + p.oP;
  const int lda = p.lda;
  if (p.L > 0)
    dense_bn_layer(X, ldx, 16 * F, p.W[0], p.b[0], p.gamma[0], p.beta[0], p.bn_rstd, p.N[0], p.ksplit[0], part, A0, lda, tid);
  if (p.L > 1)
    dense_bn_layer(A0, lda, p.N[0], p.W[1], p.b[1], p.gamma[1], p.beta[1], p.bn_rstd, p.N[1], p.ksplit[1], part, A1, lda, tid);
  if (p.L > 2)
    dense_bn_layer(A1, lda, p.N[1], p.W[2], p.b[2], p.gamma[2], p.beta[2], p.bn_rstd, p.N[2], p.ksplit[2], part, A0, lda, tid);
  // ---- the 1-unit layer, the logits layer, sigmoid: thread (r, d) of the first 256; the 16 lanes of an example are an
  // aligned group of a wave, so the xor-butterfly stays inside it ----
  if (tid < 256) {
    const int r = tid >> 4, d = tid & 15;
    const float t0 = fmaxf(ys[r] + (p.c0 != nullptr ? p.c0[0] : 0.f), 0.f);
    float z = p.wo[0] * t0 + p.wo[1] * ys[16 + r];
    if (p.L > 0) {
      const float* o = (p.L == 2 ? A1 : A0) + r * lda;
      const int NL = p.L == 1 ? p.N[0] : (p.L == 2 ? p.N[1] : p.N[2]);
      float u = 0.f;
      for (int n = d; n < NL; n += 16) u += o[n] * p.wd[n];
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) u += __shfl_xor(u, m);
      z += p.wo[2] * fmaxf(u + p.bd[0], 0.f);
    }
    z += p.bo[0];
    if (d == 0 && row0 + r < p.B) p.prob[row0 + r] = 1.f / (1.f + expf(-z));
  }
}

inline int up16(int x) { return (x + 15) & ~15; }

// LDS floats of a launch, or -1 outside the envelope.
long long predict_lds_floats(int B, int F, int D, int L, const int32_t* widths, PredictArgs* p) {
  if (D != 16 || F < 1 || F > 64 || L < 0 || L > RSX_PREDICT_MAX_LAYERS || B < 1) return -1;
  if ((long long)B * F >= (1ll << 31)) return -1;
  if (L > 0 && widths == nullptr) return -1;
  int wmax = 0;
  for (int l = 0; l < L; ++l) {
    const int n = widths[l];
    if (n < 1 || n > (1 << 20)) return -1;
    if (l + 1 < L && (n & 3)) return -1;                 // FusedTower.supports: the inner widths are multiples of 4,
    if (l + 1 == L && n > 256) return -1;                // the last one at most 256
    wmax = n > wmax ? n : wmax;
  }
  const int ldx = 16 * F + 4, lda = L > 0 ? up16(wmax) + 4 : 0;
  // partial tiles: [ksplit][16][64 * groups] of the layer that needs most; ksplit = the waves its column groups leave free
  int pmax = 0, K = 16 * F;
  for (int l = 0; l < L; ++l) {
    const int ng = (widths[l] + 63) / 64, nks = (K + 15) / 16;
    int ksp = ng >= PR_NW ? 1 : PR_NW / ng;
    ksp = ksp > nks ? nks : ksp;
    if (p) p->ksplit[l] = ksp;
    pmax = ksp * 16 * 64 * ng > pmax ? ksp * 16 * 64 * ng : pmax;
    K = widths[l];
  }
  const long long fl = 16ll * ldx + 2ll * 16 * lda + pmax + 32;
  if (fl * (long long)sizeof(float) > PR_MAX_LDS) return -1;
  if (p) {
    p->ldx = ldx;
    p->lda = lda;
    p->oA0 = 16 * ldx;
    p->oA1 = p->oA0 + 16 * lda;
    p->oP = p->oA1 + 16 * lda;
    p->oY = p->oP + pmax;
  }
  return fl;
}

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

}  // namespace

extern "C" int rsx_predict_fm_tower_supported(int B, int F, int D, int L, const int32_t* widths) {
  return predict_lds_floats(B, F, D, L, widths, nullptr) >= 0 ? 1 : 0;
}

extern "C" int rsx_predict_fm_tower(const rsx_predict_model* m, const int32_t* ids, float* prob, int B, rsx_stream_t stream) {
  if (!m || !ids || !prob || B <= 0) return RSX_EINVAL;
  if (!m->tables || !m->row_off || !m->wo || !m->bo || m->F <= 0 || m->D <= 0 || m->L < 0) return RSX_EINVAL;
  if (!(m->bn_eps >= 0.f) || !(m->bn_eps < INFINITY)) return RSX_EINVAL;
  if (m->L <= RSX_PREDICT_MAX_LAYERS) {
    for (int l = 0; l < m->L; ++l) {
      if (!m->W[l] || !m->b[l] || m->widths[l] <= 0) return RSX_EINVAL;
      if ((m->gamma[l] == nullptr) != (m->beta[l] == nullptr)) return RSX_EINVAL;
    }
    if (m->L > 0 && (!m->wd || !m->bd)) return RSX_EINVAL;
  }
  if (!al16(m->tables)) return RSX_EINVAL;               // rows are read as float4
  PredictArgs p;
  const long long fl = predict_lds_floats(B, m->F, m->D, m->L, m->widths, &p);
  if (fl < 0) return RSX_EUNSUPPORTED;
  p.tables = m->tables; p.w1 = m->w1; p.row_off = m->row_off; p.ids = ids;
  for (int l = 0; l < RSX_PREDICT_MAX_LAYERS; ++l) {
    const bool on = l < m->L;
    p.W[l] = on ? m->W[l] : nullptr; p.b[l] = on ? m->b[l] : nullptr;
    p.gamma[l] = on ? m->gamma[l] : nullptr; p.beta[l] = on ? m->beta[l] : nullptr;
    p.N[l] = on ? m->widths[l] : 0;
    if (!on) p.ksplit[l] = 1;
  }
  p.wd = m->wd; p.bd = m->bd; p.c0 = m->c0; p.wo = m->wo; p.bo = m->bo;
  p.prob = prob;
  p.w1_mask = m->w1_field_mask;
  p.bn_rstd = 1.0f / sqrtf(1.0f + m->bn_eps);
  p.B = B; p.F = m->F; p.L = m->L;
  const size_t lds = (size_t)fl * sizeof(float);
  if (lds > 64 * 1024) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(predict_fm_tower_k),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, PR_MAX_LDS);
    if (attr != hipSuccess) return RSX_EUNSUPPORTED;
  }
  RSX_LAUNCH(predict_fm_tower_k, dim3((B + PR_ROWS - 1) / PR_ROWS), dim3(PR_T), lds, rsx_s(stream), p);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
