// TF-1.x FtrlOptimizer / AdagradOptimizer on gfx950: one streaming launch over every variable segment of a step.
// Reference call sites: tf.train.FtrlOptimizer deep&wide/deep&wide.py:146-149 (estimator.LinearClassifier's default
// optimizer='Ftrl'), the FTRL-proximal trainer ftrl/ftrl.py:54; tf.train.AdagradOptimizer (the other standard embedding
// optimizer, and TF's default dnn_optimizer of the wide-and-deep estimators).
// Semantics (include/rsx.h rsx_sparse_opt_multi): TF 1.x training_ops ApplyFtrl(V2) / SparseApplyFtrl(V2) and ApplyAdagrad /
// SparseApplyAdagrad in their operation order, fp32 (-ffp-contract=off, IEEE sqrt and division).  Unlike the non-lazy Adam of
// adam.hip, the sparse forms touch only the unique rows of the step: an IndexedSlices gradient after TF's
// _apply_sparse_duplicate_indices is exactly what rsx_field_sort + rsx_segsum_bwd leave in uniq_row / nuniq / G.
//
// Memory-bound: every lane moves float4 vectors (a row of d floats is d / 4 lanes); the grid is capped and strides over the
// launch-wide work-item space of all segments.  The last workgroup advances the step word (state word 3) with the arrival
// counters of adam_device.h, so the launch replays from a HIP graph with no per-step host argument.
#include "adam_device.h"

namespace {

constexpr int SO_T = 256;               // threads per workgroup
constexpr uint32_t SO_MAX_GRID = 2048;  // 256 CUs x 8 workgroups; the rest is grid-strided

struct SoSeg {
  int32_t kind, lpr;                    // lpr: float4 per table row (TABLE_ROWS)
  long long n, begin, work;             // n as in rsx_adam_seg; work items from `begin` (a multiple of SO_T) on
  float *var, *lin, *acc, *g;
  const int32_t *slot, *uniq_row, *nuniq;
  int32_t B, stride, zero_grad, vec;    // vec: every pointer of a DENSE / VEC_SLOT segment is 16-byte aligned
};
struct SoArgs {
  SoSeg seg[RSX_ADAM_MAX_SEGS];
  int32_t nseg;
  long long chunks;                     // SO_T-item chunks of the launch (a chunk belongs to one segment)
  float* state;
  uint32_t grid;
  int32_t ftrl, sqrt_path, shrink;
  float lr, mp, l1, l2x2, l2s2;         // mp = -lr_power; l2x2 = 2 * l2; l2s2 = 2 * l2_shrinkage
};

__device__ __forceinline__ float ftrl_pow(const float x, const SoArgs& h) { return h.sqrt_path ? sqrtf(x) : powf(x, h.mp); }

// One element, TF's order of operations (include/rsx.h).
__device__ __forceinline__ void ftrl1(float& var, float& lin, float& acc, const float g, const SoArgs& h) {
  const float gs = h.shrink ? g + h.l2s2 * var : g;
  const float na = acc + g * g;
  const float pn = ftrl_pow(na, h), po = ftrl_pow(acc, h);
  lin = lin + (gs - (pn - po) / h.lr * var);
  const float y = pn / h.lr + h.l2x2;
  var = fabsf(lin) > h.l1 ? ((lin > 0.f ? h.l1 : -h.l1) - lin) / y : 0.f;
  acc = na;
}
__device__ __forceinline__ void adagrad1(float& var, float& acc, const float g, const SoArgs& h) {
  acc = acc + g * g;
  var = var - (h.lr * g) / sqrtf(acc);
}
__device__ __forceinline__ void opt1(float& var, float& lin, float& acc, const float g, const SoArgs& h) {
  if (h.ftrl) ftrl1(var, lin, acc, g, h);
  else adagrad1(var, acc, g, h);
}
// (Adagrad never reads or writes the `linear` slot: its pointer may be absent)
__device__ __forceinline__ void opt4(float4& var, float4& lin, float4& acc, const float4 g, const SoArgs& h) {
  opt1(var.x, lin.x, acc.x, g.x, h);
  opt1(var.y, lin.y, acc.y, g.y, h);
  opt1(var.z, lin.z, acc.z, g.z, h);
  opt1(var.w, lin.w, acc.w, g.w, h);
}

__device__ __forceinline__ void dense_item(const SoSeg& s, const long long e, const SoArgs& h) {
  const long long i0 = e * 4;
  if (s.vec && i0 + 4 <= s.n) {
    float4* var4 = reinterpret_cast<float4*>(s.var) + e;
    float4* acc4 = reinterpret_cast<float4*>(s.acc) + e;
    float4* g4 = reinterpret_cast<float4*>(s.g) + e;
    float4 var = *var4, acc = *acc4, lin = F4Z;
    if (h.ftrl) lin = reinterpret_cast<float4*>(s.lin)[e];
    opt4(var, lin, acc, *g4, h);
    *var4 = var;
    *acc4 = acc;
    if (h.ftrl) reinterpret_cast<float4*>(s.lin)[e] = lin;
    if (s.zero_grad) *g4 = F4Z;
    return;
  }
  const long long i1 = i0 + 4 < s.n ? i0 + 4 : s.n;
  for (long long i = i0; i < i1; ++i) {
    float var = s.var[i], acc = s.acc[i], lin = h.ftrl ? s.lin[i] : 0.f;
    opt1(var, lin, acc, s.g[i], h);
    s.var[i] = var;
    s.acc[i] = acc;
    if (h.ftrl) s.lin[i] = lin;
    if (s.zero_grad) s.g[i] = 0.f;
  }
}

// Dense form on a vector whose gradient is g[slot[i]] where slot[i] >= 0, 0 elsewhere.  all: untouched elements move too.
__device__ __forceinline__ void vec_slot_item(const SoSeg& s, const long long e, const bool all, const SoArgs& h) {
  const long long i0 = e * 4;
  if (s.vec && i0 + 4 <= s.n) {
    const int4 sl = reinterpret_cast<const int4*>(s.slot)[e];
    if (!all && (sl.x & sl.y & sl.z & sl.w) < 0) return;          // no element of the four touched
    float4 var = reinterpret_cast<float4*>(s.var)[e], acc = reinterpret_cast<float4*>(s.acc)[e], lin = F4Z;
    if (h.ftrl) lin = reinterpret_cast<float4*>(s.lin)[e];
    const float4 var0 = var, lin0 = lin, acc0 = acc;
    const float4 g = make_float4(sl.x >= 0 ? s.g[sl.x] : 0.f, sl.y >= 0 ? s.g[sl.y] : 0.f, sl.z >= 0 ? s.g[sl.z] : 0.f,
                                 sl.w >= 0 ? s.g[sl.w] : 0.f);
    opt4(var, lin, acc, g, h);
    if (!all) {      // element-wise: an untouched element keeps its bits (== its zero-gradient update, see rsx.h)
      if (sl.x < 0) { var.x = var0.x; lin.x = lin0.x; acc.x = acc0.x; }
      if (sl.y < 0) { var.y = var0.y; lin.y = lin0.y; acc.y = acc0.y; }
      if (sl.z < 0) { var.z = var0.z; lin.z = lin0.z; acc.z = acc0.z; }
      if (sl.w < 0) { var.w = var0.w; lin.w = lin0.w; acc.w = acc0.w; }
    }
    reinterpret_cast<float4*>(s.var)[e] = var;
    reinterpret_cast<float4*>(s.acc)[e] = acc;
    if (h.ftrl) reinterpret_cast<float4*>(s.lin)[e] = lin;
    return;
  }
  const long long i1 = i0 + 4 < s.n ? i0 + 4 : s.n;
  for (long long i = i0; i < i1; ++i) {
    const int sl = s.slot[i];
    if (!all && sl < 0) continue;
    float var = s.var[i], acc = s.acc[i], lin = h.ftrl ? s.lin[i] : 0.f;
    opt1(var, lin, acc, sl >= 0 ? s.g[sl] : 0.f, h);
    s.var[i] = var;
    s.acc[i] = acc;
    if (h.ftrl) s.lin[i] = lin;
  }
}

// Sparse form on one float4 of one unique row of the step (work item e of n = F*B slots x lpr lanes).
__device__ __forceinline__ void table_rows_item(const SoSeg& s, const long long e, const SoArgs& h) {
  const long long sidx = e / s.lpr;
  const int q = (int)(e - sidx * s.lpr);
  const int f = (int)(sidx / s.B), j = (int)(sidx - (long long)f * s.B);
  if (j >= s.nuniq[f]) return;
  const long long sl = (long long)f * s.stride + j;
  const long long r = (long long)s.uniq_row[sl] * s.lpr + q;
  float4 var = reinterpret_cast<float4*>(s.var)[r], acc = reinterpret_cast<float4*>(s.acc)[r], lin = F4Z;
  if (h.ftrl) lin = reinterpret_cast<float4*>(s.lin)[r];
  opt4(var, lin, acc, reinterpret_cast<const float4*>(s.g)[sl * s.lpr + q], h);
  reinterpret_cast<float4*>(s.var)[r] = var;
  reinterpret_cast<float4*>(s.acc)[r] = acc;
  if (h.ftrl) reinterpret_cast<float4*>(s.lin)[r] = lin;
}

__global__ __launch_bounds__(SO_T) void sparse_opt_k(const SoArgs a) {
  // The step this launch applies (state word 3 starts at 1).  Read before this workgroup arrives, so before the last one
  // advances it.  FTRL's untouched vector elements move at the first step (and every step under l2 shrinkage) only.
  const uint32_t step = reinterpret_cast<const uint32_t*>(a.state)[3];
  const bool vec_all = a.ftrl && (a.shrink || step == 1u);
  int si = 0;
  for (long long c = blockIdx.x; c < a.chunks; c += a.grid) {
    const long long i = c * SO_T;
    while (si + 1 < a.nseg && i >= a.seg[si + 1].begin) ++si;      // i only grows: a (workgroup-uniform) segment cursor
    const SoSeg& s = a.seg[si];
    const long long e = i - s.begin + threadIdx.x;
    if (e >= s.work) continue;
    if (s.kind == RSX_ADAM_TABLE_ROWS) table_rows_item(s, e, a);
    else if (s.kind == RSX_ADAM_DENSE) dense_item(s, e, a);
    else vec_slot_item(s, e, vec_all, a);
  }
  __syncthreads();
  if (threadIdx.x == 0 && adam_arrive_last(a.state, a.grid)) reinterpret_cast<uint32_t*>(a.state)[3] = step + 1u;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int rsx_sparse_opt_multi(const rsx_adam_seg* segs_h, int nseg, float* state, const rsx_sparse_opt_hp* hp,
                                    rsx_stream_t stream) {
  if (!segs_h || !state || !hp || nseg <= 0 || nseg > RSX_ADAM_MAX_SEGS) return RSX_EINVAL;
  SoArgs a;
  if (hp->kind != RSX_OPT_ADAGRAD && hp->kind != RSX_OPT_FTRL) return RSX_EINVAL;
  if (!(hp->lr > 0.f) || !(hp->lr < INFINITY)) return RSX_EINVAL;
  a.ftrl = hp->kind == RSX_OPT_FTRL;
  if (a.ftrl && (!(hp->lr_power <= 0.f) || !(hp->l1 >= 0.f) || !(hp->l2 >= 0.f) || !(hp->l2_shrinkage >= 0.f) ||
                 !(hp->l1 < INFINITY) || !(hp->l2 < INFINITY) || !(hp->l2_shrinkage < INFINITY)))
    return RSX_EINVAL;
  a.lr = hp->lr;
  a.sqrt_path = a.ftrl && hp->lr_power == -0.5f;
  a.shrink = a.ftrl && hp->l2_shrinkage > 0.f;
  a.mp = a.ftrl ? -hp->lr_power : 0.f;
  a.l1 = a.ftrl ? hp->l1 : 0.f;
  a.l2x2 = a.ftrl ? 2.0f * hp->l2 : 0.f;
  a.l2s2 = a.ftrl ? 2.0f * hp->l2_shrinkage : 0.f;
  a.state = state;
  long long total = 0;
  int k = 0;
  for (int i = 0; i < nseg; ++i) {
    const rsx_adam_seg& s = segs_h[i];
    if (s.n < 0 || !s.var || !s.v || !s.g || (a.ftrl && !s.m)) return RSX_EINVAL;
    for (int j = 0; j < ADAM_WMAX; ++j)
      if (s.slot_w[j]) return RSX_EINVAL;                                  // no optimizer windows here
    long long work;
    bool vec = false;
    switch (s.kind) {
      case RSX_ADAM_DENSE:
        if (s.B > 1) return RSX_EINVAL;                                    // no replica sum (single process)
        vec = al16(s.var) && al16(s.v) && al16(s.g) && (!a.ftrl || al16(s.m));
        work = (s.n + 3) >> 2;
        break;
      case RSX_ADAM_VEC_SLOT:
        if (!s.slot) return RSX_EINVAL;
        vec = al16(s.var) && al16(s.v) && al16(s.slot) && (!a.ftrl || al16(s.m));
        work = (s.n + 3) >> 2;
        break;
      case RSX_ADAM_TABLE_ROWS:
        if (!s.uniq_row || !s.nuniq || s.d < 4 || (s.d & 3) || s.g_replicas > 1) return RSX_EINVAL;
        if (s.n > 0 && (s.B <= 0 || s.stride < s.B || s.n % s.B)) return RSX_EINVAL;     // n = F * B slots (an empty batch: 0)
        if (!al16(s.var) || !al16(s.v) || !al16(s.g) || (a.ftrl && !al16(s.m))) return RSX_EINVAL;   // float4 rows
        work = s.n * (s.d >> 2);
        break;
      default: return RSX_EINVAL;                                          // TF1 / COLD / VEC_ROWS*: Adam only
    }
    if (work == 0) continue;
    SoSeg& d = a.seg[k++];
    d.kind = s.kind;
    d.lpr = s.d >> 2;
    d.n = s.n;
    d.begin = total;
    d.var = s.var;
    d.lin = s.m;
    d.acc = s.v;
    d.g = s.g;
    d.slot = s.slot;
    d.uniq_row = s.uniq_row;
    d.nuniq = s.nuniq;
    d.B = s.B;
    d.stride = s.stride;
    d.zero_grad = s.zero_grad;
    d.vec = vec ? 1 : 0;
    d.work = work;
    total += (work + SO_T - 1) / SO_T * SO_T;
  }
  a.nseg = k;
  a.chunks = total / SO_T;
  // An empty step still advances the step word (TF's global_step counts it): one workgroup with nothing to do.
  const long long want = a.chunks;
  a.grid = (uint32_t)(want < 1 ? 1 : (want > SO_MAX_GRID ? SO_MAX_GRID : want));
  RSX_LAUNCH(sparse_opt_k, dim3(a.grid), dim3(SO_T), 0, rsx_s(stream), a);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}
