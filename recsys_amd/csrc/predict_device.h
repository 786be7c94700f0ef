// What the one-launch serving kernels share.  All three (predict.hip: fm.py / deepfm.py, predict_dcn.hip: dcn.py,
// predict_din.hip: din.py's ranking): `f32x4` / `mfma16`, `up16` / `al16`, and `launch_big_lds`, the launch of a kernel that
// may need more than 64 KB of dynamic LDS.  The two tower kernels (predict.hip, predict_dcn.hip): `TowerArgs`, the tower of a
// launch with its LDS plan (`predict_lds_floats`: layout and envelope; `tower_model_valid` / `fill_tower` on the host),
// `run_tower` = the fp32 MFMA layer loop `dense_bn_layer` over a 16-example tile held in LDS, `head_dot16`, and `load_row4`, the
// one place that knows how a table row is stored (fp32, or bfloat16 / float16 widened exactly), with `dispatch_table_dtype`.
// See predict.hip's head for the layer loop's shape.
// The two gather phases stay in their kernels: they do different arithmetic on the gathered registers (fm: 8 slots, first-order
// and FM sums; dcn: NU slots, the cross layers), so a shared body would branch on its caller.
#pragma once
#include <type_traits>
#include "rsx_common.h"

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int PR_T = 512, PR_NW = PR_T / 64;   // threads / waves per workgroup
constexpr int PR_ROWS = 16;                    // examples per workgroup
constexpr int PR_GF = 8;                       // fields per gather thread: 64 fields / 8 field lanes
constexpr int PR_MAX_LDS = 160 * 1024;

inline int up16(int x) { return (x + 15) & ~15; }
inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// Launch of a kernel that may need more than 64 KB of dynamic LDS.  The raised limit is a property of a kernel FUNCTION: every
// KERNEL (so every instantiation of a kernel template) asks for its own, once.
template <auto KERNEL, class Args>
int launch_big_lds(const Args& p, const unsigned grid, const unsigned threads, const size_t lds, hipStream_t stream) {
  if (lds > 64 * 1024) {
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, PR_MAX_LDS);
    if (attr != hipSuccess) return RSX_EUNSUPPORTED;
  }
  RSX_LAUNCH(KERNEL, dim3(grid), dim3(threads), lds, stream, p);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}

// Elements 4 q .. 4 q + 3 of row `row` of tables [R, 16] stored as TD (RSX_TABLE_*), as fp32 (`load_row4`); `load_flat4` is the
// same load at a flat float4 index i = row * (D / 4) + q for the kernels whose rows are not 16 wide (predict_pair.hip).  A 16-bit
// row of 16 is 32 bytes: the thread loads the 8 bytes that hold its four elements and widens them, which is exact for both formats (subnormals, signed
// zeros included), so the kernel computes what its fp32 instantiation computes over the widened table, bit for bit.
// bfloat16 is the upper half of the fp32 pattern: a shift for the even elements, a mask for the odd ones.  float16 takes the
// hardware convert (v_cvt_f32_f16 keeps fp16 subnormals: the fp16 denormal mode is on in every HIP kernel).
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
template <int TD>
__device__ __forceinline__ f32x4 load_flat4(const void* __restrict__ tables, const size_t i) {
  if constexpr (TD == RSX_TABLE_F32) {
    return reinterpret_cast<const f32x4*>(tables)[i];
  } else if constexpr (TD == RSX_TABLE_BF16) {
    const uint2 v = reinterpret_cast<const uint2*>(tables)[i];
    return f32x4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                 __uint_as_float(v.y & 0xffff0000u)};
  } else {
    static_assert(TD == RSX_TABLE_F16, "unknown table dtype");
    return __builtin_convertvector(reinterpret_cast<const f16x4*>(tables)[i], f32x4);
  }
}
template <int TD>
__device__ __forceinline__ f32x4 load_row4(const void* __restrict__ tables, const int row, const int q) {
  return load_flat4<TD>(tables, (size_t)row * 4 + q);
}
inline bool table_dtype_known(int td) { return td == RSX_TABLE_F32 || td == RSX_TABLE_BF16 || td == RSX_TABLE_F16; }

// f(std::integral_constant<int, TD>) for the RSX_TABLE_* value td (a known one: table_dtype_known).
template <class Fn>
int dispatch_table_dtype(const int td, Fn&& f) {
  switch (td) {
    case RSX_TABLE_BF16: return f(std::integral_constant<int, RSX_TABLE_BF16>());
    case RSX_TABLE_F16: return f(std::integral_constant<int, RSX_TABLE_F16>());
    default: return f(std::integral_constant<int, RSX_TABLE_F32>());
  }
}

// The tower of a launch and the LDS plan of its tile: what predict_fm_tower_k and predict_dcn_k have in common.
struct TowerArgs {
  const float* W[RSX_PREDICT_MAX_LAYERS]; const float* b[RSX_PREDICT_MAX_LAYERS];
  const float* gamma[RSX_PREDICT_MAX_LAYERS]; const float* beta[RSX_PREDICT_MAX_LAYERS];
  float bn_rstd;                               // 1 / sqrt(1 + eps)
  int L;
  int N[RSX_PREDICT_MAX_LAYERS];
  int ksplit[RSX_PREDICT_MAX_LAYERS];          // K-splits of a layer: its column groups x ksplit work units go round the 8 waves
  int ldx, lda;                                // row strides of the gathered tile and of the activation tiles (floats, == 4 mod 8)
  int oA0, oA1, oP, oY;                        // LDS offsets (floats): activation tiles, partial tiles, the kernel's [32] slot
};

struct PredictArgs {
  const void* tables; const float* w1; const int32_t* row_off; const int32_t* ids;   // tables: [R, 16] of the kernel's TD
  TowerArgs t;                                 // t.oY: y1 | y2 [2][16]
  const float* wd; const float* bd; const float* c0; const float* wo; const float* bo;
  float* prob;
  uint64_t w1_mask;
  int B, F;
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

// The tower over the gathered tile X = lds [16][t.ldx] of K0 columns: the activation tiles ping-pong between two LDS buffers
// -> the last layer's tile [16][t.lda].  t.L == 0 (fm.py) is allowed and runs no layer; the returned pointer means something
// for t.L >= 1 only.
__device__ __forceinline__ const float* run_tower(const TowerArgs& t, float* lds, const int K0, const int tid) {
  float* A0 = lds + t.oA0;
  float* A1 = lds + t.oA1;
  float* part = lds + t.oP;
  const int lda = t.lda;
  if (t.L > 0)
    dense_bn_layer(lds, t.ldx, K0, t.W[0], t.b[0], t.gamma[0], t.beta[0], t.bn_rstd, t.N[0], t.ksplit[0], part, A0, lda, tid);
  if (t.L > 1)
    dense_bn_layer(A0, lda, t.N[0], t.W[1], t.b[1], t.gamma[1], t.beta[1], t.bn_rstd, t.N[1], t.ksplit[1], part, A1, lda, tid);
  if (t.L > 2)
    dense_bn_layer(A1, lda, t.N[1], t.W[2], t.b[2], t.gamma[2], t.beta[2], t.bn_rstd, t.N[2], t.ksplit[2], part, A0, lda, tid);
  return t.L == 2 ? A1 : A0;
}

// <o [0, N), w [0, N)> by the 16 lanes d of an example, an aligned group of a wave: n = d, d + 16, ..., then an xor butterfly
// that stays inside the group (every lane ends with the sum).
__device__ __forceinline__ float head_dot16(const float* o, const float* __restrict__ w, const int N, const int d) {
  float u = 0.f;
  for (int n = d; n < N; n += 16) u += o[n] * w[n];
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) u += __shfl_xor(u, m);
  return u;
}

// What makes a model RSX_EINVAL in the members rsx_predict_model and rsx_predict_dcn_model (M) spell alike.  Layers past
// RSX_PREDICT_MAX_LAYERS are not looked at: the arrays end there, and such an L is outside the envelope.
template <class M>
bool tower_model_valid(const M* m) {
  if (!m->tables || !m->row_off || !m->wo || !m->bo || m->F <= 0 || m->D <= 0 || m->L < 0) return false;
  if (!(m->bn_eps >= 0.f) || !(m->bn_eps < INFINITY)) return false;
  if (m->L <= RSX_PREDICT_MAX_LAYERS) {
    for (int l = 0; l < m->L; ++l) {
      if (!m->W[l] || !m->b[l] || m->widths[l] <= 0) return false;
      if ((m->gamma[l] == nullptr) != (m->beta[l] == nullptr)) return false;
    }
  }
  return table_dtype_known(m->table_dtype) && al16(m->tables);   // rows are read as float4 (16-bit rows: 8 bytes of a 32-byte row)
}

// The model's part of a TowerArgs that predict_lds_floats has planned (so m->L <= RSX_PREDICT_MAX_LAYERS).
template <class M>
void fill_tower(TowerArgs* t, const M* m) {
  for (int l = 0; l < RSX_PREDICT_MAX_LAYERS; ++l) {
    const bool on = l < m->L;
    t->W[l] = on ? m->W[l] : nullptr; t->b[l] = on ? m->b[l] : nullptr;
    t->gamma[l] = on ? m->gamma[l] : nullptr; t->beta[l] = on ? m->beta[l] : nullptr;
    t->N[l] = on ? m->widths[l] : 0;
    if (!on) t->ksplit[l] = 1;
  }
  t->bn_rstd = 1.0f / sqrtf(1.0f + m->bn_eps);
  t->L = m->L;
}

// LDS floats of a launch, or -1 outside the envelope.
inline long long predict_lds_floats(int B, int F, int D, int L, const int32_t* widths, TowerArgs* p) {
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

// The same plan for the pair ranker (predict_pair.hip): a tile of 16 (user, item) pairs whose gathered row is K0 = 2 D wide,
// D in {8, 16, 32} -- predict_lds_floats' plan with 2 D in place of 16 F, which is its plan for F = D / 8 fields of 16.
inline long long pair_lds_floats(int U, int C, int D, int L, const int32_t* widths, TowerArgs* p) {
  if ((D != 8 && D != 16 && D != 32) || L < 1 || U < 1 || C < 1) return -1;
  if ((long long)U * C >= (1ll << 31)) return -1;
  return predict_lds_floats(1, D / 8, 16, L, widths, p);
}

}  // namespace
