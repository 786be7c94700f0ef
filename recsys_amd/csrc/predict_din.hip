// Candidate ranking of din.py as ONE launch: one user history against C candidates -> prob [U, C] (include/rsx.h
// rsx_predict_din_rank).  Reference: din/din.py:83-140 in PREDICT mode, for every (candidate, that user's history) example: the
// two lookups of the target (:100-101), both `_attention` blocks with their own 80-40-1 weights (:103-125, mask id > 0 at ANY
// position, dropout off), 'mlp_layer' 100-50-20-1 (:130-138) and + i_item[i_id] (:139), sigmoid.
//
// The first attention layer is folded.  With W0 = [Wh; Wq; Wp; Wm] (four K-row blocks)
//     concat[h, q, h*q, h-q] . W0 = h . (Wh + Wm) + q . (Wq - Wm) + (h*q) . Wp
// the first term belongs to the user (one row per history position), the second to the candidate, and only the third, a K-deep
// product, to the (candidate, position) pair.  Wh + Wm and Wq - Wm are formed here, from the variables, on every call: the kernel
// follows a reloaded model with no host-side state.
//
// A workgroup (8 waves) owns one user and CT consecutive candidates (CT = 1 .. 8, chosen by the host from U * C so that small
// requests still spread over the chip; nothing a pair computes depends on CT):
//   0  the history ids of both tables are compacted (positions with id > 0, in order): padding costs no matrix work
//   1  the valid history rows are fetched ONCE into LDS (H [2][rows][K + 4]), the candidates' rows beside them
//   2  Uu = H . (Wh + Wm) per table (MFMA, row tiles of 16 over the table's 4 waves) and Vb = q . (Wq - Wm) + b0 per candidate
//   3  waves 0-3 serve the item history, 4-7 the category history; a wave keeps ITS table's Wp, W1, b1, W2 in registers (~125
//      VGPRs) for the whole phase and takes (candidate, 16-position tile) units in turn.  Everything is computed TRANSPOSED
//      (weights are the MFMA A operand, the 16 pairs the B operand's columns), so that a layer's accumulator tile IS the next
//      layer's B operand (v_mfma_f32_16x16x4_f32: D row 4 kq + r of column i <-> B k = 4 kq + t of column i): no LDS round
//      trip between the layers.  The 1-unit layer is a per-lane dot product + two cross-lane adds, the masked weighted sum
//      of the tile four butterfly steps; a unit leaves K partial sums in LDS
//   4  the tiles' partial sums are added in tile order -> the tower's input [q_item | pooled item | pooled category]
//   5  the tower, again transposed MFMA tiles (weights from L2 straight into A operands), bias, + i_item, sigmoid
// No atomics, no workspace; every sum has a fixed order that does not involve C, the candidate's position, U or its
// neighbours, so a pair's bits depend on its ids and the model only.
#include "rsx_common.h"
#include "predict_device.h"      // f32x4, mfma16, up16, al16, launch_big_lds

namespace {
constexpr int DR_T = 512, DR_NW = DR_T / 64;
constexpr int DR_N1 = 80, DR_N2 = 40;          // attention widths (din/din.py:85)
constexpr int DR_T1 = DR_N1 / 16, DR_T2 = (DR_N2 + 15) / 16;
constexpr int DR_PMAX = 128, DR_CT_MAX = 8, DR_MAXTILES = DR_PMAX / 16;
constexpr int DR_LDU = DR_N1 + 4;
constexpr int DR_M0 = 100, DR_M1 = 50, DR_M2 = 20;                     // 'mlp_layer' widths (din/din.py:86)
constexpr int DR_LDA1 = 116, DR_LDA2 = 68, DR_LDA3 = 36;                // activation row strides (width rounded up to 16, + 4)

struct DinRankArgs {
  const float* tab[2];                         // item rows, category rows [., K]
  const float* bias; int bias_ld;
  const float* aW0[2]; const float* ab0[2]; const float* aW1[2]; const float* ab1[2]; const float* aW2[2]; const float* ab2[2];
  const float* mW[3]; const float* mb[3]; int mld[3];
  const float* wout; const float* bout;
  const int32_t* hist[2]; const int32_t* cand[2];
  float* prob;
  int U, C, P, CT, ctiles, PT;                 // PT = P rounded up to 16
  int oH, oU, oQ, oV, oPP, oX, oA1, oA2, oA3, oVid;   // LDS offsets (floats)
};

// One tower layer, transposed: out [c][n] = relu(sum_k in [c][k] W [k][n] + b [n]), n < N; the columns N .. up16(N) of out become
// zeros (the next layer's last k-step reads them).  A wave takes 16-row tiles of W^T; D row 4 kq + r = unit 16 tile + 4 kq + r of
// column i = candidate i.  Candidates past nc read the last one's row and store nothing.
template <int KS>
__device__ __forceinline__ void tower_layer(const float* __restrict__ in, const int ldi, const int Kin, const float* __restrict__ W,
                                            const int ldw, const float* __restrict__ b, const int N, float* __restrict__ out,
                                            const int ldo, const int nc, const int w, const int lane) {
  const int i = lane & 15, kq = lane >> 4;
  const int ci = i < nc ? i : nc - 1;
  const int ntile = (N + 15) >> 4;
  for (int tile = w; tile < ntile; tile += DR_NW) {           // (wave-uniform)
    const int n = 16 * tile + i, nn = n < N ? n : N - 1;
    float a[KS][4];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = 16 * ks + 4 * kq + t;
        const float v = W[(k < Kin ? k : Kin - 1) * ldw + nn];
        a[ks][t] = k < Kin ? v : 0.f;
      }
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float4 x = *reinterpret_cast<const float4*>(in + ci * ldi + 16 * ks + 4 * kq);
      acc = mfma16(a[ks][0], x.x, acc);
      acc = mfma16(a[ks][1], x.y, acc);
      acc = mfma16(a[ks][2], x.z, acc);
      acc = mfma16(a[ks][3], x.w, acc);
    }
    if (i < nc) {
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * tile + 4 * kq + r;
        o[r] = m < N ? fmaxf(acc[r] + b[m < N ? m : N - 1], 0.f) : 0.f;
      }
      *reinterpret_cast<f32x4*>(out + i * ldo + 16 * tile + 4 * kq) = o;
    }
  }
}

// SHARED: every user is scored against the SAME C candidates (cand [C], row stride 0: rsx_predict_din_rank_shared).  An
// instantiation of its own, so the per-user form compiles to the code it had before the shared one existed.
template <int K, bool SHARED>
__global__ __launch_bounds__(DR_T) void predict_din_rank_k(const DinRankArgs p) {
  constexpr int KS = K / 16, K4 = K / 4, LDH = K + 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int i = lane & 15, kq = lane >> 4;
  const int u = blockIdx.x / p.ctiles;
  const int c0 = (blockIdx.x - u * p.ctiles) * p.CT;
  const int nc = p.C - c0 < p.CT ? p.C - c0 : p.CT;
  const int cbase = (SHARED ? 0 : u * p.C) + c0;   // where this workgroup's candidates start in cand
  const int P = p.P, PT = p.PT, CT = p.CT;
  float* Hs = lds + p.oH;                      // [2][PT][LDH]  valid history rows, compacted
  float* Us = lds + p.oU;                      // [2][PT][DR_LDU]  H . (Wh + Wm)
  float* Qs = lds + p.oQ;                      // [2][CT][K]  the candidates' rows
  float* Vs = lds + p.oV;                      // [2][CT][DR_N1]  q . (Wq - Wm) + b0
  float* PPs = lds + p.oPP;                    // [2][CT][DR_MAXTILES][K]  partial weighted sums
  float* Xs = lds + p.oX;                      // [CT][3 K]
  float* A1 = lds + p.oA1;
  float* A2 = lds + p.oA2;
  float* A3 = lds + p.oA3;
  int* vid = reinterpret_cast<int*>(lds + p.oVid);   // [2][PT] ids of the valid positions | [2] their number
  int* nvs = vid + 2 * PT;

  // ---- 0: compaction of both histories (wave a = table a) ----
  if (w < 2) {
    const int32_t* __restrict__ h = p.hist[w] + u * P;
    int base = 0;
    for (int p0 = 0; p0 < P; p0 += 64) {
      const int pos = p0 + lane;
      const int id = pos < P ? h[pos] : 0;
      const bool ok = id > 0;
      const unsigned long long m = __ballot(ok);
      if (ok) vid[w * PT + base + __popcll(m & ((1ull << lane) - 1ull))] = id;
      base += __popcll(m);
    }
    if (lane == 0) nvs[w] = base;
  }
  __syncthreads();
  const int nv0 = nvs[0], nv1 = nvs[1];
  // ---- 1: history rows (once per workgroup; the rows that fill the last tile are zeros) and candidate rows ----
  for (int e = tid; e < 2 * PT * K4; e += DR_T) {
    const int a = e / (PT * K4), rem = e - a * (PT * K4);
    const int j = rem / K4, q4 = rem - j * K4;
    const int nv = a ? nv1 : nv0;
    if (j < ((nv + 15) & ~15)) {
      float4 v = F4Z;
      if (j < nv) v = *reinterpret_cast<const float4*>(p.tab[a] + (size_t)vid[a * PT + j] * K + 4 * q4);
      *reinterpret_cast<float4*>(Hs + (a * PT + j) * LDH + 4 * q4) = v;
    }
  }
  for (int e = tid; e < 2 * CT * K4; e += DR_T) {
    const int a = e / (CT * K4), rem = e - a * (CT * K4);
    const int c = rem / K4, q4 = rem - c * K4;
    const int cc = c < nc ? c : nc - 1;
    const int id = p.cand[a][cbase + cc];
    const float4 v = *reinterpret_cast<const float4*>(p.tab[a] + (size_t)id * K + 4 * q4);
    *reinterpret_cast<float4*>(Qs + (a * CT + c) * K + 4 * q4) = v;
    if (a == 0) *reinterpret_cast<float4*>(Xs + c * 3 * K + 4 * q4) = v;
  }
  __syncthreads();
  const int a = w >> 2, wl = w & 3;             // this wave's table, its index among the table's 4 waves
  const int nv = a ? nv1 : nv0;
  const int ntile = (nv + 15) >> 4;
  const float* __restrict__ W0 = p.aW0[a];
  // ---- 2: Vb (thread = (table, candidate, unit)) and Uu (MFMA row tiles) ----
  for (int o = tid; o < 2 * nc * DR_N1; o += DR_T) {
    const int ta = o / (nc * DR_N1), rem = o - ta * (nc * DR_N1);
    const int c = rem / DR_N1, n = rem - c * DR_N1;
    const float* __restrict__ Wa = p.aW0[ta];
    const float* q = Qs + (ta * CT + c) * K;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) acc = fmaf(q[k], Wa[(K + k) * DR_N1 + n] - Wa[(3 * K + k) * DR_N1 + n], acc);
    Vs[(ta * CT + c) * DR_N1 + n] = acc + p.ab0[ta][n];
  }
  if (wl < ntile) {
    float whm[KS][4][DR_T1];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) {
          const int k = 16 * ks + 4 * kq + t;
          whm[ks][t][tl] = W0[k * DR_N1 + 16 * tl + i] + W0[(3 * K + k) * DR_N1 + 16 * tl + i];
        }
    for (int tt = wl; tt < ntile; tt += 4) {
      f32x4 acc[DR_T1];
#pragma unroll
      for (int tl = 0; tl < DR_T1; ++tl) acc[tl] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const float4 h = *reinterpret_cast<const float4*>(Hs + (a * PT + 16 * tt + i) * LDH + 16 * ks + 4 * kq);
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) acc[tl] = mfma16(whm[ks][0][tl], h.x, acc[tl]);
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) acc[tl] = mfma16(whm[ks][1][tl], h.y, acc[tl]);
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) acc[tl] = mfma16(whm[ks][2][tl], h.z, acc[tl]);
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) acc[tl] = mfma16(whm[ks][3][tl], h.w, acc[tl]);
      }
#pragma unroll
      for (int tl = 0; tl < DR_T1; ++tl)
        *reinterpret_cast<f32x4*>(Us + (a * PT + 16 * tt + i) * DR_LDU + 16 * tl + 4 * kq) = acc[tl];
    }
  }
  __syncthreads();
  // ---- 3: the (candidate, position tile) units of this wave's table ----
  const int nunit = nc * ntile;
  if (wl < nunit) {
    float wp[KS][4][DR_T1];                      // Wp^T: A operands of the first layer
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl)
          wp[ks][t][tl] = W0[(2 * K + 16 * ks + 4 * kq + t) * DR_N1 + 16 * tl + i];
    const float* __restrict__ W1 = p.aW1[a];
    float w1[DR_T1][4][DR_T2];                   // W1^T: A operands of the second layer (units past 40: zeros)
#pragma unroll
    for (int ks = 0; ks < DR_T1; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int t2 = 0; t2 < DR_T2; ++t2) {
          const int n2 = 16 * t2 + i;
          const float v = W1[(16 * ks + 4 * kq + t) * DR_N2 + (n2 < DR_N2 ? n2 : DR_N2 - 1)];
          w1[ks][t][t2] = n2 < DR_N2 ? v : 0.f;
        }
    float b1[DR_T2][4], w2[DR_T2][4];            // by accumulator element: unit 16 t2 + 4 kq + r
#pragma unroll
    for (int t2 = 0; t2 < DR_T2; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n2 = 16 * t2 + 4 * kq + r, nn = n2 < DR_N2 ? n2 : DR_N2 - 1;
        const float bv = p.ab1[a][nn], wv = p.aW2[a][nn];
        b1[t2][r] = n2 < DR_N2 ? bv : 0.f;
        w2[t2][r] = n2 < DR_N2 ? wv : 0.f;
      }
    const float b2 = p.ab2[a][0];
    for (int un = wl; un < nunit; un += 4) {     // (wave-uniform)
      const int c = un / ntile, tt = un - c * ntile;
      const float* hrow = Hs + (a * PT + 16 * tt + i) * LDH + 4 * kq;
      const float* qrow = Qs + (a * CT + c) * K + 4 * kq;
      float4 hv[KS];
      f32x4 acc0[DR_T1];
#pragma unroll
      for (int tl = 0; tl < DR_T1; ++tl) acc0[tl] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        hv[ks] = *reinterpret_cast<const float4*>(hrow + 16 * ks);
        const float4 x = f4_mul(hv[ks], *reinterpret_cast<const float4*>(qrow + 16 * ks));
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) acc0[tl] = mfma16(wp[ks][0][tl], x.x, acc0[tl]);
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) acc0[tl] = mfma16(wp[ks][1][tl], x.y, acc0[tl]);
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) acc0[tl] = mfma16(wp[ks][2][tl], x.z, acc0[tl]);
#pragma unroll
        for (int tl = 0; tl < DR_T1; ++tl) acc0[tl] = mfma16(wp[ks][3][tl], x.w, acc0[tl]);
      }
      // a1 = relu(pair term + (user term + candidate term)): accumulator element r of tile tl is unit 16 tl + 4 kq + r
      const float* urow = Us + (a * PT + 16 * tt + i) * DR_LDU + 4 * kq;
      const float* vrow = Vs + (a * CT + c) * DR_N1 + 4 * kq;
      f32x4 acc1[DR_T2];
#pragma unroll
      for (int t2 = 0; t2 < DR_T2; ++t2) acc1[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int tl = 0; tl < DR_T1; ++tl) {
        const float4 uu = *reinterpret_cast<const float4*>(urow + 16 * tl);
        const float4 vb = *reinterpret_cast<const float4*>(vrow + 16 * tl);
        const float a0 = fmaxf(acc0[tl][0] + (uu.x + vb.x), 0.f), a1 = fmaxf(acc0[tl][1] + (uu.y + vb.y), 0.f);
        const float a2 = fmaxf(acc0[tl][2] + (uu.z + vb.z), 0.f), a3 = fmaxf(acc0[tl][3] + (uu.w + vb.w), 0.f);
#pragma unroll
        for (int t2 = 0; t2 < DR_T2; ++t2) acc1[t2] = mfma16(w1[tl][0][t2], a0, acc1[t2]);
#pragma unroll
        for (int t2 = 0; t2 < DR_T2; ++t2) acc1[t2] = mfma16(w1[tl][1][t2], a1, acc1[t2]);
#pragma unroll
        for (int t2 = 0; t2 < DR_T2; ++t2) acc1[t2] = mfma16(w1[tl][2][t2], a2, acc1[t2]);
#pragma unroll
        for (int t2 = 0; t2 < DR_T2; ++t2) acc1[t2] = mfma16(w1[tl][3][t2], a3, acc1[t2]);
      }
      float s = 0.f;
#pragma unroll
      for (int t2 = 0; t2 < DR_T2; ++t2)
#pragma unroll
        for (int r = 0; r < 4; ++r) s = fmaf(fmaxf(acc1[t2][r] + b1[t2][r], 0.f), w2[t2][r], s);
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      const float wgt = 16 * tt + i < nv ? s + b2 : 0.f;          // the rows that fill the last tile weigh nothing
      float pv[KS][4];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        pv[ks][0] = hv[ks].x * wgt; pv[ks][1] = hv[ks].y * wgt; pv[ks][2] = hv[ks].z * wgt; pv[ks][3] = hv[ks].w * wgt;
      }
#pragma unroll
      for (int m = 1; m < 16; m <<= 1)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int e = 0; e < 4; ++e) pv[ks][e] += __shfl_xor(pv[ks][e], m);
      if (i == 0) {
        float* pp = PPs + ((a * CT + c) * DR_MAXTILES + tt) * K + 4 * kq;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<float4*>(pp + 16 * ks) = make_float4(pv[ks][0], pv[ks][1], pv[ks][2], pv[ks][3]);
      }
    }
  }
  __syncthreads();
  // ---- 4: pooled histories, tiles in order ----
  for (int e = tid; e < 2 * nc * K; e += DR_T) {
    const int ta = e / (nc * K), rem = e - ta * (nc * K);
    const int c = rem / K, k = rem - c * K;
    const int nt = ((ta ? nv1 : nv0) + 15) >> 4;
    float s = 0.f;
    for (int t = 0; t < nt; ++t) s += PPs[((ta * CT + c) * DR_MAXTILES + t) * K + k];
    Xs[c * 3 * K + (1 + ta) * K + k] = s;
  }
  __syncthreads();
  // ---- 5: the tower and the head ----
  tower_layer<3 * K / 16>(Xs, 3 * K, 3 * K, p.mW[0], p.mld[0], p.mb[0], DR_M0, A1, DR_LDA1, nc, w, lane);
  __syncthreads();
  tower_layer<(DR_M0 + 15) / 16>(A1, DR_LDA1, DR_M0, p.mW[1], p.mld[1], p.mb[1], DR_M1, A2, DR_LDA2, nc, w, lane);
  __syncthreads();
  tower_layer<(DR_M1 + 15) / 16>(A2, DR_LDA2, DR_M1, p.mW[2], p.mld[2], p.mb[2], DR_M2, A3, DR_LDA3, nc, w, lane);
  __syncthreads();
  if (tid < nc) {
    const float* x = A3 + tid * DR_LDA3;
    float z = 0.f;
#pragma unroll
    for (int n = 0; n < DR_M2; ++n) z = fmaf(x[n], p.wout[n], z);
    const int id = p.cand[0][cbase + tid];
    z = (z + p.bout[0]) + p.bias[(size_t)id * p.bias_ld];
    p.prob[u * p.C + c0 + tid] = 1.f / (1.f + expf(-z));
  }
}

bool din_rank_envelope(int U, int C, int P, int K, int n1, int n2, int L, const int32_t* widths) {
  if (U < 1 || C < 1 || P < 1 || P > DR_PMAX) return false;
  if (K != 16 && K != 32) return false;
  if (n1 != DR_N1 || n2 != DR_N2 || L != 3 || widths == nullptr) return false;
  if (widths[0] != DR_M0 || widths[1] != DR_M1 || widths[2] != DR_M2) return false;
  if ((long long)U * C * P >= (1ll << 31)) return false;
  return true;
}

// Candidates per workgroup: as many workgroups as the chip has compute units before a workgroup takes a second candidate.
inline int din_rank_ct(int U, int C) {
  const long long pairs = (long long)U * C;
  long long ct = (pairs + 255) / 256;
  ct = ct < 1 ? 1 : (ct > DR_CT_MAX ? DR_CT_MAX : ct);
  return (int)(ct < C ? ct : C);
}

size_t din_rank_layout(DinRankArgs* p, int K) {
  const int PT = p->PT, CT = p->CT;
  int o = 0;
  p->oH = o; o += 2 * PT * (K + 4);
  p->oU = o; o += 2 * PT * DR_LDU;
  p->oQ = o; o += 2 * CT * K;
  p->oV = o; o += 2 * CT * DR_N1;
  p->oPP = o; o += 2 * CT * DR_MAXTILES * K;
  p->oX = o; o += CT * 3 * K;
  p->oA1 = o; o += CT * DR_LDA1;
  p->oA2 = o; o += CT * DR_LDA2;
  p->oA3 = o; o += CT * DR_LDA3;
  p->oVid = o; o += 2 * PT + 4;
  return (size_t)o * sizeof(float);
}

}  // namespace

extern "C" int rsx_predict_din_rank_supported(int U, int C, int P, int K, int n1, int n2, int L, const int32_t* widths) {
  return din_rank_envelope(U, C, P, K, n1, n2, L, widths) ? 1 : 0;
}

namespace {
int din_rank_launch(const rsx_predict_din_model* m, const int32_t* hist_item, const int32_t* hist_cate, const int32_t* cand_item,
                    const int32_t* cand_cate, float* prob, int U, int C, int P, bool shared, rsx_stream_t stream) {
  if (!m || !hist_item || !hist_cate || !cand_item || !cand_cate || !prob || U <= 0 || C <= 0 || P <= 0) return RSX_EINVAL;
  if (!m->item_emb || !m->cate_emb || !m->item_bias || !m->mlp_wout || !m->mlp_bout) return RSX_EINVAL;
  if (m->K <= 0 || m->n1 <= 0 || m->n2 <= 0 || m->L < 0 || m->bias_ld < 1) return RSX_EINVAL;
  for (int a = 0; a < 2; ++a)
    for (int l = 0; l < 3; ++l)
      if (!m->att_W[a][l] || !m->att_b[a][l]) return RSX_EINVAL;
  if (m->L <= RSX_PREDICT_MAX_LAYERS)
    for (int l = 0; l < m->L; ++l)
      if (!m->mlp_W[l] || !m->mlp_b[l] || m->widths[l] <= 0 || m->ld[l] < m->widths[l]) return RSX_EINVAL;
  if (!al16(m->item_emb) || !al16(m->cate_emb)) return RSX_EINVAL;      // rows are read as float4
  if (!din_rank_envelope(U, C, P, m->K, m->n1, m->n2, m->L, m->widths)) return RSX_EUNSUPPORTED;
  DinRankArgs p;
  p.tab[0] = m->item_emb; p.tab[1] = m->cate_emb;
  p.bias = m->item_bias; p.bias_ld = m->bias_ld;
  for (int a = 0; a < 2; ++a) {
    p.aW0[a] = m->att_W[a][0]; p.ab0[a] = m->att_b[a][0];
    p.aW1[a] = m->att_W[a][1]; p.ab1[a] = m->att_b[a][1];
    p.aW2[a] = m->att_W[a][2]; p.ab2[a] = m->att_b[a][2];
  }
  for (int l = 0; l < 3; ++l) { p.mW[l] = m->mlp_W[l]; p.mb[l] = m->mlp_b[l]; p.mld[l] = m->ld[l]; }
  p.wout = m->mlp_wout; p.bout = m->mlp_bout;
  p.hist[0] = hist_item; p.hist[1] = hist_cate; p.cand[0] = cand_item; p.cand[1] = cand_cate;
  p.prob = prob;
  p.U = U; p.C = C; p.P = P;
  p.CT = din_rank_ct(U, C);
  p.ctiles = (C + p.CT - 1) / p.CT;
  p.PT = up16(P);
  const size_t lds = din_rank_layout(&p, m->K);
  if (lds > (size_t)PR_MAX_LDS) return RSX_EUNSUPPORTED;
  const unsigned grid = (unsigned)(U * p.ctiles);
  if (shared)
    return m->K == 32 ? launch_big_lds<predict_din_rank_k<32, true>>(p, grid, DR_T, lds, rsx_s(stream))
                      : launch_big_lds<predict_din_rank_k<16, true>>(p, grid, DR_T, lds, rsx_s(stream));
  return m->K == 32 ? launch_big_lds<predict_din_rank_k<32, false>>(p, grid, DR_T, lds, rsx_s(stream))
                    : launch_big_lds<predict_din_rank_k<16, false>>(p, grid, DR_T, lds, rsx_s(stream));
}
}  // namespace

extern "C" int rsx_predict_din_rank(const rsx_predict_din_model* m, const int32_t* hist_item, const int32_t* hist_cate,
                                    const int32_t* cand_item, const int32_t* cand_cate, float* prob, int U, int C, int P,
                                    rsx_stream_t stream) {
  return din_rank_launch(m, hist_item, hist_cate, cand_item, cand_cate, prob, U, C, P, false, stream);
}

extern "C" int rsx_predict_din_rank_shared(const rsx_predict_din_model* m, const int32_t* hist_item, const int32_t* hist_cate,
                                           const int32_t* cand_item, const int32_t* cand_cate, float* prob, int U, int C, int P,
                                           rsx_stream_t stream) {
  return din_rank_launch(m, hist_item, hist_cate, cand_item, cand_cate, prob, U, C, P, true, stream);
}
