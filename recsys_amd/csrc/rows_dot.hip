// Dot products of rows of one fp32 matrix (include/rsx.h rsx_rows_dot): scores[q, j] = dot(unit[q_rows[q]], unit[first + j])
// for Q query rows against n consecutive rows of unit [N, K], K in {16, 32}.  serving.Predictor.build_neighbours runs it over
// the unit-length item embeddings of the resident catalogue, chunk by chunk, with rsx_topk_rows_excl behind every chunk.
//
// ARITHMETIC (the contract; serving.rows_dot_host restates it in numpy): one fp32 accumulator per output,
//     s = +0.0f; for d = 0 .. K - 1: s = s + a[d] * b[d]
// ascending in d, every product and every sum rounded to fp32, no fused multiply-add (the build passes -ffp-contract=off) and
// no matrix-core instruction, whose internal summation order could not be restated.  No split accumulators.
//
// TILE: a workgroup of 256 threads takes 64 query rows x 256 catalogue rows.  The query rows go to LDS once (8 KB at K = 32).
// A thread owns ONE catalogue row, loaded with K / 4 16-byte loads into registers, and walks the query rows 128 / K at a time
// (K = 16: eight, K = 32: four): that many independent accumulators, so the K-long dependent chain of one output is hidden
// behind the others and behind the workgroup's other waves.  Every lane of a wave reads the same query element at the same time
// -- one LDS address, a broadcast, no bank conflict -- and one 16-byte LDS read feeds eight vector instructions.  A thread's
// outputs of a pass go to as many rows of `scores`, each store 256 B per wave.
// REGISTERS: the compiler issues all LDS reads of a pass ahead of its arithmetic, 128 / K x K / 4 = 32 reads of 16 bytes, 128
// registers, in either form (146 and 162 in all: three waves per SIMD).  Eight query rows a pass at K = 32 were 292 registers, one
// wave per SIMD -- and a wave alone on its SIMD issues a vector instruction every 4 cycles instead of every 2.
// The work is N^2 K multiplies and as many adds on the vector ALUs; the catalogue rows are re-read once per 64 queries, from L2.
// A q_rows entry outside [0, N) is treated as a row of zeros: no address is formed from it.
#include "rsx_common.h"

namespace {

constexpr int RD_T = 256;      // threads = catalogue rows of a workgroup
constexpr int RD_QB = 64;      // query rows of a workgroup

struct RowsDotArgs {
  const float4* unit;
  const int32_t* q_rows;
  float* scores;
  int N, Q, first, n, ld;
};

template <int K>
__global__ __launch_bounds__(RD_T, 2) void rows_dot_k(const RowsDotArgs p) {
  constexpr int K4 = K / 4;
  constexpr int RD_QI = 128 / K;                      // outputs a thread computes at a time; divides RD_QB
  __shared__ float4 qs[RD_QB * K4];
  const int tid = threadIdx.x;
  const int q0 = blockIdx.y * RD_QB;
  const int nq = p.Q - q0 < RD_QB ? p.Q - q0 : RD_QB;
  for (int t = tid; t < RD_QB * K4; t += RD_T) {
    const int r = t / K4, c = t - r * K4;
    float4 v = F4Z;
    if (r < nq) {
      const int row = p.q_rows[q0 + r];
      if (row >= 0 && row < p.N) v = p.unit[(size_t)row * K4 + c];
    }
    qs[t] = v;
  }
  const int j = blockIdx.x * RD_T + tid;
  const bool ok = j < p.n;
  float4 b[K4];
  const float4* src = p.unit + (size_t)(p.first + (ok ? j : 0)) * K4;
#pragma unroll
  for (int c = 0; c < K4; ++c) b[c] = src[c];
  __syncthreads();
  for (int qb = 0; qb < nq; qb += RD_QI) {            // (rows nq .. of the tile are zeros: computed, never stored)
    float acc[RD_QI];
#pragma unroll
    for (int i = 0; i < RD_QI; ++i) acc[i] = 0.f;
#pragma unroll
    for (int c = 0; c < K4; ++c) {
#pragma unroll
      for (int i = 0; i < RD_QI; ++i) {
        const float4 a = qs[(qb + i) * K4 + c];
        acc[i] = acc[i] + a.x * b[c].x;
        acc[i] = acc[i] + a.y * b[c].y;
        acc[i] = acc[i] + a.z * b[c].z;
        acc[i] = acc[i] + a.w * b[c].w;
      }
    }
    if (ok) {
#pragma unroll
      for (int i = 0; i < RD_QI; ++i)
        if (qb + i < nq) p.scores[(size_t)(q0 + qb + i) * p.ld + j] = acc[i];
    }
  }
}

inline bool rows_dot_envelope(int K) { return K == 16 || K == 32; }

}  // namespace

extern "C" int rsx_rows_dot_supported(int K) { return rows_dot_envelope(K) ? 1 : 0; }

extern "C" int rsx_rows_dot(const float* unit, int N, int K, const int32_t* q_rows, int Q, int first, int n, float* scores, int ld,
                            rsx_stream_t stream) {
  if (!unit || !q_rows || !scores || N <= 0 || K <= 0 || Q <= 0 || n <= 0 || first < 0 || (long long)first + n > N || ld < n)
    return RSX_EINVAL;
  if (reinterpret_cast<uintptr_t>(unit) & 15u) return RSX_EINVAL;
  if (!rows_dot_envelope(K)) return RSX_EUNSUPPORTED;
  const long long gy = ((long long)Q + RD_QB - 1) / RD_QB;
  if (gy > 65535) return RSX_EUNSUPPORTED;
  RowsDotArgs p;
  p.unit = reinterpret_cast<const float4*>(unit); p.q_rows = q_rows; p.scores = scores;
  p.N = N; p.Q = Q; p.first = first; p.n = n; p.ld = ld;
  const dim3 grid((unsigned)((n + RD_T - 1) / RD_T), (unsigned)gy);
  if (K == 16) RSX_LAUNCH(rows_dot_k<16>, grid, dim3(RD_T), 0, rsx_s(stream), p);
  else RSX_LAUNCH(rows_dot_k<32>, grid, dim3(RD_T), 0, rsx_s(stream), p);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
