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
#include "predict_device.h"

namespace {
// TD: how the table rows are stored (RSX_TABLE_*); only the row load differs between the instantiations.
template <int TD>
__global__ __launch_bounds__(PR_T) void predict_fm_tower_k(const PredictArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS;
  const int F = p.F, ldx = p.t.ldx;
  float* X = lds;                                        // [16][ldx]: the examples' rows, field-major (= E.reshape(B, F * 16))
  float* ys = lds + p.t.oY;                              // y1 [16] | y2 [16]
  // ---- gather + first-order sum + FM term (the lane mapping of gather_device.h on half a wave per example): thread =
  // (example r, field lane j, float4 quarter q), fields j, j + 8, ...; ids and offsets first, then every row load, then the
  // stores and sums in ascending f.  Rows past the batch take the last example's ids (never ids past B); their outputs are
  // not stored. ----
  {
    const int r = tid >> 5, j = (tid >> 2) & 7, q = tid & 3;
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
      ev[u] = load_row4<TD>(p.tables, row[u], q);
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
  // ---- the tower, then the 1-unit layer, the logits layer, sigmoid: thread (r, d) of the first 256 ----
  const float* AL = run_tower(p.t, lds, 16 * F, tid);
  if (tid < 256) {
    const int r = tid >> 4, d = tid & 15;
    const float t0 = fmaxf(ys[r] + (p.c0 != nullptr ? p.c0[0] : 0.f), 0.f);
    float z = p.wo[0] * t0 + p.wo[1] * ys[16 + r];
    if (p.t.L > 0) {
      const int NL = p.t.L == 1 ? p.t.N[0] : (p.t.L == 2 ? p.t.N[1] : p.t.N[2]);
      z += p.wo[2] * fmaxf(head_dot16(AL + r * p.t.lda, p.wd, NL, d) + p.bd[0], 0.f);
    }
    z += p.bo[0];
    if (d == 0 && row0 + r < p.B) p.prob[row0 + r] = 1.f / (1.f + expf(-z));
  }
}

}  // namespace

extern "C" int rsx_predict_fm_tower_supported(int B, int F, int D, int L, const int32_t* widths) {
  return predict_lds_floats(B, F, D, L, widths, nullptr) >= 0 ? 1 : 0;
}

extern "C" int rsx_predict_fm_tower(const rsx_predict_model* m, const int32_t* ids, float* prob, int B, rsx_stream_t stream) {
  if (!m || !ids || !prob || B <= 0 || !tower_model_valid(m)) return RSX_EINVAL;
  if (m->L > 0 && m->L <= RSX_PREDICT_MAX_LAYERS && (!m->wd || !m->bd)) return RSX_EINVAL;
  PredictArgs p;
  const long long fl = predict_lds_floats(B, m->F, m->D, m->L, m->widths, &p.t);
  if (fl < 0) return RSX_EUNSUPPORTED;
  fill_tower(&p.t, m);
  p.tables = m->tables; p.w1 = m->w1; p.row_off = m->row_off; p.ids = ids;
  p.wd = m->wd; p.bd = m->bd; p.c0 = m->c0; p.wo = m->wo; p.bo = m->bo;
  p.prob = prob;
  p.w1_mask = m->w1_field_mask;
  p.B = B; p.F = m->F;
  const unsigned grid = (B + PR_ROWS - 1) / PR_ROWS;
  const size_t lds = (size_t)fl * sizeof(float);
  return dispatch_table_dtype(m->table_dtype, [&](auto td) {
    return launch_big_lds<predict_fm_tower_k<decltype(td)::value>>(p, grid, PR_T, lds, rsx_s(stream));
  });
}
