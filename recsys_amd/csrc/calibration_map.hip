// Isotonic calibration on gfx950 (include/rsx.h rsx_calibration_quantile_table, rsx_calibrate_apply): the equal-mass, tie-aware
// table an isotonic map is fitted from, reduced from the sorted keys csrc/auc_exact.hip leaves on the device, and the map itself,
// applied to a batch of probabilities.  Opt-in; it changes nothing of csrc/calibration.hip or csrc/auc_exact.hip.
//
// THE CONTRACT OF THE TABLE, in integers.  ks[0 .. V) are the sorted valid keys of rsx_auc_exact_append, (bits(p) << 1) | positive
// (the padding keys lie behind them and are never read).  h(i) is the position of the first key with i's score (key >> 1), the
// bin of position i is b(i) = (h(i) * M) / V in 64-bit integers: all examples of one score share a bin, bins ascend with the score,
// bins may be empty (heavy ties, M > V).  Row b = {count, positives, q_sum} with q = uint64(double(p) * 2^32), calibration.hip's row
// and q, so metrics.calibration_from_table reduces this table too.  The host divides (metrics.isotonic_from_table).
//
// THE TABLE KERNEL.  One workgroup of 256 threads per bin; no atomics, no workspace, nothing zeroed by the caller.  The positions
// with b(i) >= b are those whose head is at or behind t_b = ceil(b V / M): they start at t_b when t_b is a head (or 0, or V) and
// otherwise behind the tie group that holds t_b, found by a binary search for the first key of a larger score in (t_b, V].  Bin b
// is [start(b), start(b + 1)): thread 0 finds both ends (two searches of <= 27 dependent loads), the workgroup strides over the
// range -- a scalar head up to 16-byte alignment, uint4 loads, a scalar tail -- sums in 64 bits per thread, reduces through
// shuffles and LDS in a fixed order, and one lane stores the three words.  Integer sums: the table depends on neither batch
// sizes, batch order nor the order threads run in.  With all scores equal ONE workgroup reads everything: slow (one CU's load
// rate) but correct; DESIGN.md section 11c has the measured price.
//
// THE MAP, in fp32 (compiled with -ffp-contract=off and IEEE division).  Knots x[0 .. K) strictly increasing, y[0 .. K)
// non-decreasing, 1 <= K <= 1024.  A p outside [0, 1] by the example rule of csrc/eval_device.h (-0.0 counts as +0.0) is returned
// unchanged, bit for bit.  p <= x[0] -> y[0]; p >= x[K-1] -> y[K-1]; otherwise with j the largest index with x[j] <= p
//     t = (p - x[j]) / (x[j+1] - x[j]);  o = y[j] + t * (y[j+1] - y[j]);  out = o < y[j+1] ? o : y[j+1]
// one subtraction on each side, one division, one multiply, one add, one minimum, in that order.
//
// THE APPLY KERNEL.  256 threads; a bounded grid strides over n.  Every workgroup stages the knots in LDS once (8 KiB at 1024
// knots); an element is a binary search in LDS (<= 10 steps) and the five operations.  When prob_in and prob_out share their
// offset within 16 bytes the body moves float4s behind a scalar head and in front of a scalar tail; otherwise every element is a
// scalar.  Every element is read and written by the same thread: prob_out may equal prob_in (it may not overlap it otherwise).
// Nothing is allocated and nothing synchronises: the launch can be captured into a graph.
#include "rsx_common.h"
#include "eval_device.h"      // the example rule, q, the workgroup reduction

namespace {
constexpr int CM_T = 256;
constexpr int CM_W = CM_T / RSX_WAVE;
constexpr int CM_MAX_BINS = 1024;         // rsx_calibration_max_bins()
constexpr int CM_MAX_KNOTS = 1024;
constexpr int CM_APPLY_MAX_GRID = 1024;

// first position at or behind t whose key is a head (V when there is none); t <= V
__device__ int64_t cm_first_head(const uint32_t* __restrict__ ks, int64_t V, int64_t t) {
  if (t <= 0) return 0;
  if (t >= V) return V;
  const uint32_t s = ks[t] >> 1;
  if ((ks[t - 1] >> 1) != s) return t;
  int64_t lo = t + 1, hi = V;             // the first i in [lo, hi] with score(i) > s; hi == V stands for "none"
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((ks[mid] >> 1) > s) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ void cm_take(uint32_t k, ull& pos, ull& q) {
  pos += k & 1u;
  q += ev_q(k >> 1);
}

__global__ __launch_bounds__(CM_T) void cm_quantile_table_k(const uint32_t* __restrict__ ks, int64_t V, int M,
                                                            ull* __restrict__ table) {
  __shared__ int64_t range[2];
  __shared__ ull lpos[CM_W], lq[CM_W];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid < 2) {
    const int bb = b + tid;
    range[tid] = bb >= M ? V : cm_first_head(ks, V, ((int64_t)bb * V + M - 1) / M);
  }
  __syncthreads();
  const int64_t lo = range[0], hi = range[1];
  ull pos = 0ull, q = 0ull;
  int64_t a0 = (lo + 3) & ~(int64_t)3;    // keys is 16-byte aligned: positions that are multiples of 4 are uint4 boundaries
  if (a0 > hi) a0 = hi;
  const int64_t a1 = a0 + ((hi - a0) & ~(int64_t)3);
  if (lo + tid < a0) cm_take(ks[lo + tid], pos, q);
  for (int64_t i = a0 + 4 * (int64_t)tid; i < a1; i += 4 * CM_T) {
    const uint4 v = *reinterpret_cast<const uint4*>(ks + i);
    cm_take(v.x, pos, q);
    cm_take(v.y, pos, q);
    cm_take(v.z, pos, q);
    cm_take(v.w, pos, q);
  }
  if (a1 + tid < hi) cm_take(ks[a1 + tid], pos, q);
  const ull p = ev_block_reduce<false, CM_W>(pos, lpos), s = ev_block_reduce<false, CM_W>(q, lq);
  if (tid == 0) {
    table[3 * b] = (ull)(hi - lo);
    table[3 * b + 1] = p;
    table[3 * b + 2] = s;
  }
}

__device__ __forceinline__ float cm_map(float p, const float* sx, const float* sy, int K) {
  const EvExample e = ev_example(p, 0.f);
  if (!e.valid) return p;                 // outside [0, 1], NaN, infinities: unchanged, bit for bit
  const float v = __uint_as_float(e.u);   // -0.0 is +0.0
  if (v <= sx[0]) return sy[0];
  if (v >= sx[K - 1]) return sy[K - 1];
  int lo = 0, hi = K - 1;                 // x[lo] <= v < x[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (sx[mid] <= v) lo = mid; else hi = mid;
  }
  const float x0 = sx[lo], y0 = sy[lo], y1 = sy[hi];
  const float t = (v - x0) / (sx[hi] - x0);
  const float o = y0 + t * (y1 - y0);
  return o < y1 ? o : y1;
}

__global__ __launch_bounds__(CM_T) void cm_apply_k(const float* __restrict__ x, const float* __restrict__ y, int K,
                                                   const float* in, float* out, int64_t n, int64_t head) {
  __shared__ float sx[CM_MAX_KNOTS], sy[CM_MAX_KNOTS];
  float vx[CM_MAX_KNOTS / CM_T], vy[CM_MAX_KNOTS / CM_T];   // every load issued before the first is waited for
#pragma unroll
  for (int r = 0; r < CM_MAX_KNOTS / CM_T; ++r) {
    const int i = r * CM_T + threadIdx.x;
    vx[r] = i < K ? x[i] : 0.f;
    vy[r] = i < K ? y[i] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < CM_MAX_KNOTS / CM_T; ++r) {
    const int i = r * CM_T + threadIdx.x;
    if (i < K) {
      sx[i] = vx[r];
      sy[i] = vy[r];
    }
  }
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * CM_T + threadIdx.x, stride = (int64_t)gridDim.x * CM_T;
  const int64_t body = (n - head) & ~(int64_t)3;           // head == n: no vector body at all
  for (int64_t i = g; i < head; i += stride) out[i] = cm_map(in[i], sx, sy, K);
  for (int64_t i = head + 4 * g; i < head + body; i += 4 * stride) {
    float4 v = *reinterpret_cast<const float4*>(in + i);
    v.x = cm_map(v.x, sx, sy, K);
    v.y = cm_map(v.y, sx, sy, K);
    v.z = cm_map(v.z, sx, sy, K);
    v.w = cm_map(v.w, sx, sy, K);
    *reinterpret_cast<float4*>(out + i) = v;
  }
  for (int64_t i = head + body + g; i < n; i += stride) out[i] = cm_map(in[i], sx, sy, K);
}
}  // namespace

extern "C" int rsx_calibration_quantile_table(const uint32_t* sorted_keys, int64_t n_valid, int n_bins, uint64_t* table,
                                              rsx_stream_t stream) {
  if (!sorted_keys || !table || n_valid < 0 || n_valid > rsx_auc_exact_max_keys()) return RSX_EINVAL;
  if (n_bins < 2 || n_bins > CM_MAX_BINS) return RSX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(sorted_keys) & 15u) || (reinterpret_cast<uintptr_t>(table) & 7u)) return RSX_EINVAL;
  RSX_LAUNCH(cm_quantile_table_k, dim3((unsigned)n_bins), dim3(CM_T), 0, rsx_s(stream), sorted_keys, n_valid, n_bins,
             reinterpret_cast<ull*>(table));
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}

extern "C" int rsx_calibrate_apply(const float* x, const float* y, int n_knots, const float* prob_in, float* prob_out, int64_t n,
                                   rsx_stream_t stream) {
  if (!x || !y || !prob_in || !prob_out || n < 0 || n_knots < 1 || n_knots > CM_MAX_KNOTS) return RSX_EINVAL;
  const uintptr_t ai = reinterpret_cast<uintptr_t>(prob_in), ao = reinterpret_cast<uintptr_t>(prob_out);
  if ((ai & 3u) || (ao & 3u) || (reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(y) & 3u)) return RSX_EINVAL;
  if (n == 0) return RSX_OK;
  int64_t head = n;                        // the offsets within 16 bytes differ: every element is a scalar
  if ((ai & 15u) == (ao & 15u)) {
    head = (int64_t)(((16u - (ai & 15u)) & 15u) >> 2);
    if (head > n) head = n;
  }
  int64_t blocks = (n + 4 * CM_T - 1) / (4 * CM_T);
  if (blocks > CM_APPLY_MAX_GRID) blocks = CM_APPLY_MAX_GRID;
  RSX_LAUNCH(cm_apply_k, dim3((unsigned)blocks), dim3(CM_T), 0, rsx_s(stream), x, y, n_knots, prob_in, prob_out, n, head);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
