// What the kernels on the bf16 matrix cores share: csrc/cin_bf16.hip, csrc/cin_bf16_wide.hip, csrc/cin_split.hip, csrc/din_attn.hip.
//   * the operand vector types, the 16x16x32 bf16 MFMA, one-quad operand loads, bf16 pair packing;
//   * split operands: v_mfma_f32_16x16x32_bf16 multiplies its 8-bit-significand operands EXACTLY and accumulates in fp32 at 16x
//     the rate of v_mfma_f32_16x16x4_f32.  An fp32 number is the exact sum of three bf16 numbers (x = x1 + x2 + x3, x1 = bf16(x),
//     x2 = bf16(x - x1), x3 = x - x1 - x2), so a product of two fp32 numbers is the sum of nine exact bf16 products; the six with
//     i + j <= 4 carry everything above 2^-24 of the product: fp32-grade, 6 MFMAs = 3/8 of the fp32 MFMA's time;
//   * StageX0: the CIN kernels' X0 rows of a workgroup's examples on their way to LDS;
//   * host side: rup, the opt-in for more than 64 KiB of dynamic LDS, the k-step dispatcher.
#pragma once
#include <type_traits>
#include "rsx_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16_t;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 ld_bf16x8(const bf16_t* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p));
}
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  bf16x2 v;
  v[0] = (bf16_t)lo;
  v[1] = (bf16_t)hi;
  return __builtin_bit_cast(uint32_t, v);
}

// two fp32 values -> 3 packed bf16 pairs: plane s holds bf16 of what the planes before it left over
__device__ __forceinline__ void split2(float lo, float hi, uint32_t (&out)[3]) {
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const uint32_t pk = pack2(lo, hi);
    out[s] = pk;
    if (s + 1 < 3) {
      lo -= __uint_as_float(pk << 16);
      hi -= __uint_as_float(pk & 0xffff0000u);
    }
  }
}
// eight fp32 values (two float4) -> 3 operand quads (element j of the quad = value j)
__device__ __forceinline__ void split8(float4 a, float4 b, bf16x8 (&out)[3]) {
  uint32_t p0[3], p1[3], p2[3], p3[3];
  split2(a.x, a.y, p0);
  split2(a.z, a.w, p1);
  split2(b.x, b.y, p2);
  split2(b.z, b.w, p3);
#pragma unroll
  for (int s = 0; s < 3; ++s) out[s] = __builtin_bit_cast(bf16x8, (u32x4){p0[s], p1[s], p2[s], p3[s]});
}
// T += sum over the six kept plane products (smallest first: lvl = i + j, zero based, is 2^-8lvl in relative size) and the KS
// k-steps of a-plane x b-plane; a is the MFMA's first operand (rows), b its second (columns) -- BA: the other way round, the
// products in the same order
template <int KS, bool BA = false>
__device__ __forceinline__ f32x4 split_mma(const bf16x8 (&a)[3][KS], const bf16x8 (&b)[3][KS], f32x4 T) {
#pragma unroll
  for (int lvl = 2; lvl >= 0; --lvl)
#pragma unroll
    for (int sa = 0; sa <= lvl; ++sa)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) T = BA ? mfma_bf16(b[lvl - sa][ks], a[sa][ks], T) : mfma_bf16(a[sa][ks], b[lvl - sa][ks], T);
  return T;
}
// (one k-step, the planes as plain arrays)
__device__ __forceinline__ f32x4 split_mma(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 T) {
  return split_mma<1>(reinterpret_cast<const bf16x8(&)[3][1]>(a), reinterpret_cast<const bf16x8(&)[3][1]>(b), T);
}

// X0 [B, F, 16] of a workgroup's E examples (64 E threads) -> LDS [E][FP * 16], zeros for the fields F .. FP - 1 (a field past
// F multiplies by zero: no bounds tests in the field loops): 3 float4 per thread (E * 160 items), requested together
template <int E>
struct StageX0 {
  static constexpr int D = 16, FP = 40, NTHR = 64 * E;
  float4 v[3];
  __device__ __forceinline__ void load(const float* X0, int b0, int B, int F, int tid) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int e4 = tid + NTHR * u;
      const int ex = e4 / (FP * 4), r = e4 % (FP * 4);
      // (unconditional loads from clamped addresses, zeroed afterwards: a load under a condition becomes a branch, and the
      // compiler waits for each of them in turn)
      const int exc = ex < E ? ex : E - 1;
      const bool ok = e4 < E * FP * 4 && (r >> 2) < F && b0 + ex < B;
      const int bc = b0 + exc < B ? b0 + exc : B - 1, rc = (r >> 2) < F ? r : 0;
      const float4 t = reinterpret_cast<const float4*>(X0 + (size_t)bc * F * D)[rc];
      v[u] = make_float4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
    }
  }
  __device__ __forceinline__ void store(float* sX0, int tid) const {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int e4 = tid + NTHR * u;
      if (e4 < E * FP * 4) reinterpret_cast<float4*>(sX0)[e4] = v[u];
    }
  }
};

// -------------------------------------------------------------------------------------------------------------- host side
inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// gfx950 has 160 KiB of LDS per CU; above 64 KiB a kernel must opt in (host-side attribute, no stream work)
template <typename K>
int opt_in_lds(K kernel, size_t lds) {
  if (lds > 160 * 1024) return RSX_EUNSUPPORTED;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return RSX_ELAUNCH;
  return RSX_OK;
}

// f(integral_constant<int, KS>) for KS = ks clamped to 1..4: the k-steps (32 elements each) of a contraction over <= 128 padded
// rows as a template parameter
template <typename Fn>
int dispatch_ks(const int ks, Fn&& f) {
  switch (ks) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    default: return f(std::integral_constant<int, 4>());
  }
}
