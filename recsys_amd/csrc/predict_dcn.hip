// Serving forward of dcn.py as ONE launch: ids [B, F] -> prob [B] (include/rsx.h rsx_predict_dcn).
// Reference: dcn/dcn.py:123-153 in PREDICT mode (input_layer lookup x0 [B, 16 F]; Lc cross layers x_{l+1} = (x_l . w_l) * x0 +
// x_l + b_l; the tower over x0, L x [dense(relu) -> batch_normalization(training=False) -> dropout(training=False)] with no
// 1-unit layer on top; logit = concat[tower_out, x_Lc] . out.W + out.b; sigmoid).  No first-order term and no FM term.
//
// The shape is predict_fm_tower_k's (predict.hip): 512 threads own 16 examples from the ids to the probability, thread =
// (example r, field lane j, float4 quarter q) gathers fields j, j + 8, ... into registers and into the LDS tile X, the first
// MFMA A operand of `dense_bn_layer` (predict_device.h).  What is new is the cross phase.  It runs on the registers the gather
// threads hold (NU float4 of x0 per thread): per layer a thread loads its slice of w_l and b_l, forms its partial dot product
// in ascending field order, and the 32 threads of the example -- an aligned half wave -- sum it with a fixed xor butterfly
// (fp32 addition commutes, so every lane ends with the same bits); x_{l+1} is formed in registers.  The same reduction over
// out.W[widths[L-1]:] gives cz = <x_Lc, out.W[widths[L-1]:]> into a [16] LDS slot, and the head is
// z = <tower_out, out.W[:widths[L-1]]> + cz + out.b.  Slots of fields past F hold exact zeros in x0, w, b alike.
// The arithmetic is cross_device.h's (dot4's pairing, (s * x0 + x) + b), on another lane layout.
// w_{l+1} (after the last layer: the out.W slice) is loaded before layer l's reduction and b_l at the layer's top, so a
// layer waits for no load but its first.  out.W[widths[L-1]:] is 16-byte aligned only when the last width is a multiple of
// 4: otherwise it is read with 4-byte loads (a wave-uniform choice).
// No workspace, no atomics, no allocation, no sync: a row's bits depend on its own ids and the model only.
#include "rsx_common.h"
#include "predict_device.h"

namespace {

constexpr int DCN_MAX_LC = 8;                  // cross.hip's CROSS_MAX_L

struct PredictDcnArgs {
  const void* tables; const int32_t* row_off; const int32_t* ids;   // tables: [R, 16] of the kernel's TD
  TowerArgs t;                                 // t.L >= 1; t.oY: cz [16]
  const float* cw; const float* cb;            // cross.W, cross.b [Lc][16 F] (16-byte aligned)
  const float* wo; const float* bo;            // out.W [t.N[t.L-1] + 16 F], out.b [1]
  float* prob;
  int B, F, Lc;
};

// v[u] = the 4 floats at base + off[u]: one 16-byte load each (VEC: base 16-byte aligned; off[u] is a multiple of 4) or four
// 4-byte loads.
template <int NU>
__device__ __forceinline__ void load_slices(f32x4 (&v)[NU], const float* __restrict__ base, const int (&off)[NU], const bool vec) {
  if (vec) {
#pragma unroll
    for (int u = 0; u < NU; ++u) v[u] = *reinterpret_cast<const f32x4*>(base + off[u]);
  } else {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[u][e] = base[off[u] + e];
    }
  }
}

// Sum over the 32 threads of an example (an aligned half wave): the same bits in every lane.
__device__ __forceinline__ float half_wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// NU: float4 slots per gather thread = fields j, j + 8, ..., j + 8 (NU - 1); 8 NU >= F.  TD: how the table rows are stored
// (RSX_TABLE_*); only the row load differs.
template <int NU, int TD>
__global__ __launch_bounds__(PR_T) void predict_dcn_k(const PredictDcnArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS;
  const int F = p.F, ldx = p.t.ldx;
  float* X = lds;                                        // [16][ldx]: the examples' rows, field-major (= x0)
  float* czs = lds + p.t.oY;                             // cz [16]
  const int NL = p.t.N[p.t.L - 1];                       // the last width: out.W = [tower part NL | cross part 16 F]
  // ---- gather (predict_fm_tower_k's mapping) + the cross layers on the gathered registers.  Rows past the batch take the
  // last example's ids (never ids past B); their outputs are not stored. ----
  {
    const int r = tid >> 5, j = (tid >> 2) & 7, q = tid & 3;
    const int b = row0 + r < p.B ? row0 + r : p.B - 1;
    const uint32_t ib = (uint32_t)b * (uint32_t)F;
    const int dim = 16 * F;
    const float* __restrict__ wox = p.wo + NL;                // out.W's cross part [16 F]
    const bool wox_vec = (reinterpret_cast<uintptr_t>(wox) & 15u) == 0;
    int row[NU], off[NU];                                // off: this thread's float offset inside a [16 F] vector (clamped)
    bool on[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int f = j + 8 * u;
      const int fc = f < F ? f : F - 1;
      on[u] = f < F;
      off[u] = fc * 16 + q * 4;
      row[u] = p.row_off[fc] + p.ids[ib + (uint32_t)fc];
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 x0[NU], wc[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) x0[u] = load_row4<TD>(p.tables, row[u], q);
    load_slices<NU>(wc, p.cw, off, true);                // w_0
    __builtin_amdgcn_sched_barrier(0);                   // (every load in flight before the first store)
    f32x4 x[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (on[u]) *reinterpret_cast<f32x4*>(X + r * ldx + off[u]) = x0[u];
      x0[u] = on[u] ? x0[u] : zero;
      x[u] = x0[u];
    }
    for (int l = 0; l < p.Lc; ++l) {
      f32x4 bb[NU], wn[NU];
      load_slices<NU>(bb, p.cb + (size_t)l * dim, off, true);
      if (l + 1 < p.Lc) load_slices<NU>(wn, p.cw + (size_t)(l + 1) * dim, off, true);
      else load_slices<NU>(wn, wox, off, wox_vec);
      float part = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const f32x4 w = on[u] ? wc[u] : zero;
        part += (x[u][0] * w[0] + x[u][1] * w[1]) + (x[u][2] * w[2] + x[u][3] * w[3]);
      }
      const float s = half_wave_sum(part);
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const f32x4 bu = on[u] ? bb[u] : zero;
        x[u] = (s * x0[u] + x[u]) + bu;
        wc[u] = wn[u];
      }
    }
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const f32x4 w = on[u] ? wc[u] : zero;
      part += (x[u][0] * w[0] + x[u][1] * w[1]) + (x[u][2] * w[2] + x[u][3] * w[3]);
    }
    const float cz = half_wave_sum(part);
    if ((tid & 31) == 0) czs[r] = cz;
  }
  __syncthreads();
  // ---- the tower, then the logits layer, sigmoid: thread (r, d) of the first 256 ----
  // predict_dcn_lds_floats refuses L < 1 before any launch: run_tower's first layer needs no guard here.  An envelope that
  // lets L = 0 through must drop this line.
  __builtin_assume(p.t.L >= 1);
  const float* AL = run_tower(p.t, lds, 16 * F, tid);
  if (tid < 256) {
    const int r = tid >> 4, d = tid & 15;
    const float z = (head_dot16(AL + r * p.t.lda, p.wo, NL, d) + czs[r]) + p.bo[0];
    if (d == 0 && row0 + r < p.B) p.prob[row0 + r] = 1.f / (1.f + expf(-z));
  }
}

// LDS floats of a launch (predict_fm_tower's plan: the cz slot takes the place of y1 | y2), or -1 outside the envelope.
long long predict_dcn_lds_floats(int B, int F, int D, int L, const int32_t* widths, int Lc, TowerArgs* plan) {
  if (L < 1 || Lc < 1 || Lc > DCN_MAX_LC) return -1;
  return predict_lds_floats(B, F, D, L, widths, plan);
}

}  // namespace

extern "C" int rsx_predict_dcn_supported(int B, int F, int D, int L, const int32_t* widths, int Lc) {
  return predict_dcn_lds_floats(B, F, D, L, widths, Lc, nullptr) >= 0 ? 1 : 0;
}

extern "C" int rsx_predict_dcn(const rsx_predict_dcn_model* m, const int32_t* ids, float* prob, int B, rsx_stream_t stream) {
  if (!m || !ids || !prob || B <= 0 || !tower_model_valid(m)) return RSX_EINVAL;
  if (m->Lc < 0 || !m->cross_W || !m->cross_b || !al16(m->cross_W) || !al16(m->cross_b)) return RSX_EINVAL;   // read as float4
  PredictDcnArgs p;
  const long long fl = predict_dcn_lds_floats(B, m->F, m->D, m->L, m->widths, m->Lc, &p.t);
  if (fl < 0) return RSX_EUNSUPPORTED;
  fill_tower(&p.t, m);
  p.tables = m->tables; p.row_off = m->row_off; p.ids = ids;
  p.cw = m->cross_W; p.cb = m->cross_b; p.wo = m->wo; p.bo = m->bo;
  p.prob = prob;
  p.B = B; p.F = m->F; p.Lc = m->Lc;
  const unsigned grid = (B + PR_ROWS - 1) / PR_ROWS;
  const size_t lds = (size_t)fl * sizeof(float);
  return dispatch_table_dtype(m->table_dtype, [&](auto td) {
    constexpr int TD = decltype(td)::value;    // fields per gather thread: 5 covers F <= 40 (Criteo-39), 8 every F of the envelope
    return p.F <= 40 ? launch_big_lds<predict_dcn_k<5, TD>>(p, grid, PR_T, lds, rsx_s(stream))
                     : launch_big_lds<predict_dcn_k<8, TD>>(p, grid, PR_T, lds, rsx_s(stream));
  });
}
