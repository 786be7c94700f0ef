// Calibration tables on gfx950 (include/rsx.h rsx_calibration_*): what a reliability table, ECE / MCE, predicted-over-observed CTR
// and their per-slice forms are made of, accumulated on the device beside the rank statistics of csrc/metrics.hip,
// csrc/auc_exact.hip and csrc/auc_group.hip.  Opt-in; it changes none of them.
//
// THE CONTRACT, in integers.  An example is (fp32 p, label y[, group g]).  Whether it is positive and whether p is valid
// (0 <= p <= 1) is the example rule of csrc/eval_device.h, as is q below; with a group column the example is valid only when
// 0 <= g < n_groups too.  An invalid example enters no table and is counted.  Of a valid example
//     bin  b = min(n_bins - 1, int(p * float(n_bins)))     ONE fp32 multiply, rounded to nearest, then truncated: the arithmetic is
//                                                          the definition (a p one ulp below k / n_bins may land in bin k)
//     q    = uint64(double(p) * 2^32)                      the product is exact in fp64; the conversion truncates; q <= 2^32
// and every table row is three 64-bit integers {count, positives, q_sum}: bins[b] and group_table[g].  Sums of q hold 2^31 examples.
// The HOST divides (metrics.calibration_from_table).  Integer adds commute: the tables depend on neither batch sizes, batch order
// nor the order threads run in.
//
// THE KERNEL.  One launch per eval batch fills both tables: 256 threads, at most CAL_MAX_GRID workgroups that stride over the
// examples (prob / labels loads coalesced; the group column read in place through its element stride, as auc_group.hip's append
// reads it).  Bin table: a histogram in LDS -- 32-bit LDS integer atomics for count and positives, one 64-bit LDS integer atomic for
// q_sum, 16 KB at 1024 bins -- and, behind a barrier, one non-returning 64-bit global integer atomic per NON-ZERO entry
// (metrics.hip's flush).  A workgroup sees at most ceil(n / gridDim) <= 2^23 examples of a launch (n <= CAL_MAX_N), so its 32-bit
// counts cannot wrap.  Group table: 64-bit global integer atomics on group_table[3 g + {0, 1, 2}]; a negative adds nothing to
// positives and a zero q nothing to q_sum.  The invalid count: one atomic per workgroup.  No allocation, no workspace, no
// synchronisation, nothing zeroed: the caller zeroes the state once.
#include "rsx_common.h"
#include "eval_device.h"      // the example rule, q, the group-id test, the invalid-count flush

namespace {
constexpr int CAL_T = 256;
constexpr int CAL_MAX_BINS = 1024;
constexpr int64_t CAL_MAX_GROUPS = 1ll << 22;
constexpr int CAL_MAX_GRID = 256;
constexpr int64_t CAL_MAX_N = 1ll << 31;

__global__ __launch_bounds__(CAL_T) void cal_update_k(const float* __restrict__ prob, const float* __restrict__ labels,
                                                      const int32_t* __restrict__ groups, int64_t gstride, int64_t n, int n_bins,
                                                      uint32_t n_groups, ull* bins, ull* group_table, ull* invalid_word) {
  __shared__ unsigned int h_count[CAL_MAX_BINS], h_pos[CAL_MAX_BINS];
  __shared__ ull h_q[CAL_MAX_BINS];
  for (int i = threadIdx.x; i < n_bins; i += CAL_T) {
    h_count[i] = 0u;
    h_pos[i] = 0u;
    h_q[i] = 0ull;
  }
  __syncthreads();
  const float fbins = (float)n_bins;
  unsigned int wave_bad = 0u;
  for (int64_t i = (int64_t)blockIdx.x * CAL_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * CAL_T) {
    const EvExample e = ev_example(prob[i], labels[i]);
    const int32_t g = n_groups ? groups[i * gstride] : 0;
    const bool bad = !e.valid || (n_groups && !ev_group_ok(g, n_groups));
    wave_bad += ev_count_invalid(bad);
    if (bad) continue;
    const bool pos = e.pos;
    const float p = __uint_as_float(e.u);
    const ull q = ev_q(e.u);
    if (n_bins) {
      int b = (int)(p * fbins);
      b = b < n_bins - 1 ? b : n_bins - 1;
      atomicAdd(&h_count[b], 1u);
      if (pos) atomicAdd(&h_pos[b], 1u);
      if (q) atomicAdd(&h_q[b], q);
    }
    if (n_groups) {
      ull* row = group_table + (size_t)g * 3;
      atomicAdd(row, 1ull);
      if (pos) atomicAdd(row + 1, 1ull);
      if (q) atomicAdd(row + 2, q);
    }
  }
  ev_flush_invalid<CAL_T / 64>(wave_bad, invalid_word);      // its barrier stands between the LDS atomics above and the reads below
  for (int i = threadIdx.x; i < n_bins; i += CAL_T) {
    if (h_count[i]) atomicAdd(&bins[3 * i], (ull)h_count[i]);
    if (h_pos[i]) atomicAdd(&bins[3 * i + 1], (ull)h_pos[i]);
    if (h_q[i]) atomicAdd(&bins[3 * i + 2], h_q[i]);
  }
}
}  // namespace

extern "C" int rsx_calibration_max_bins(void) { return CAL_MAX_BINS; }

extern "C" int rsx_calibration_max_groups(void) { return (int)CAL_MAX_GROUPS; }

extern "C" int rsx_calibration_update(const float* prob, const float* labels, const int32_t* groups, int64_t group_stride, int64_t n,
                                      int n_bins, int64_t n_groups, uint64_t* bins, uint64_t* group_table, uint64_t* invalid,
                                      rsx_stream_t stream) {
  if (!prob || !labels || !invalid || n < 0 || n_bins < 0 || n_groups < 0) return RSX_EINVAL;
  if (n_bins == 0 && n_groups == 0) return RSX_EINVAL;    // no table to fill
  if (n_bins && !bins) return RSX_EINVAL;
  if (n_groups && (!groups || !group_table || group_stride < 1)) return RSX_EINVAL;
  if (n_bins == 1 || n_bins > CAL_MAX_BINS || n_groups > CAL_MAX_GROUPS || n > CAL_MAX_N) return RSX_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(bins) & 7u) || (reinterpret_cast<uintptr_t>(group_table) & 7u) ||
      (reinterpret_cast<uintptr_t>(invalid) & 7u))
    return RSX_EINVAL;
  if (n == 0) return RSX_OK;
  int64_t blocks = (n + CAL_T - 1) / CAL_T;
  if (blocks > CAL_MAX_GRID) blocks = CAL_MAX_GRID;
  RSX_LAUNCH(cal_update_k, dim3((unsigned)blocks), dim3(CAL_T), 0, rsx_s(stream), prob, labels, groups, group_stride, n, n_bins,
             (uint32_t)n_groups, reinterpret_cast<ull*>(bins), reinterpret_cast<ull*>(group_table), reinterpret_cast<ull*>(invalid));
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
