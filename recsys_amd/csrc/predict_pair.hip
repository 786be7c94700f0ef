// Item ranking of an exported two-field deepfm.py model (u_id, i_id) as ONE launch: U users, C items each -> prob [U, C]
// (include/rsx.h rsx_predict_pair_rank).  Reference: deepfm/deepfm.py:85-113 in PREDICT mode on the example (user, item);
// the arithmetic is predict.hip's (first-order sum, FM term, run_tower, the 1-unit layer, the logits layer, sigmoid) with the
// embedding size as a template parameter: the gathered row is X = [e_0 | e_1], K0 = 2 D wide, D in {8, 16, 32}.
//
// A workgroup owns 16 consecutive items of ONE user.  Thread (pair r, float4 quarter q) of the first 16 * D / 4 loads its
// quarter of BOTH rows: the 16 pairs read the user's row and its w1 entry from the same address (one cache line per workgroup;
// the bits are those of a single fetch), the item rows go straight into the LDS tile [16][2 D + 4].  With both slots in one
// thread the sums over the slots need no exchange: s = e_0 + e_1, qq = e_0^2 + e_1^2 in ascending slot order, then the
// butterfly over the D / 4 quarters -- at D = 16 the order of predict_fm_tower_k for F = 2.
// The user's half of layer 0 (e_u . W0[user rows], the same for the 16 pairs) is NOT folded: DESIGN.md 10f prices it.
#include "rsx_common.h"
#include "predict_device.h"

namespace {
struct PairArgs {
  const void* tables; const float* w1; const int32_t* row_off;      // tables: [R, D] of the kernel's TD
  const int32_t* user_id; const int32_t* item_id;
  TowerArgs t;                                 // t.oY: y1 | y2 [2][16]
  const float* wd; const float* bd; const float* c0; const float* wo; const float* bo;
  float* prob;
  uint64_t w1_mask;
  int U, C, item_ld, user_slot, tiles;         // tiles = ceil(C / 16): workgroups per user
};

template <int TD, int D>
__global__ __launch_bounds__(PR_T) void predict_pair_rank_k(const PairArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DQ = D / 4;                              // float4 quarters of a row
  const int tid = threadIdx.x;
  const int u = blockIdx.x / p.tiles, c0 = (blockIdx.x % p.tiles) * PR_ROWS;
  const int ldx = p.t.ldx;
  float* X = lds;                                        // [16][ldx]: slot 0's row | slot 1's row
  float* ys = lds + p.t.oY;                              // y1 [16] | y2 [16]
  // ---- gather + first-order sum + FM term: rows past C take the last candidate's id; their outputs are not stored ----
  if (tid < PR_ROWS * DQ) {                              // (32 / 64 / 128 threads: whole quarter groups of a wave)
    const int r = tid / DQ, q = tid % DQ;
    const int c = c0 + r < p.C ? c0 + r : p.C - 1;
    const int uid = p.user_id[u];
    const int iid = p.item_id[(size_t)u * (size_t)p.item_ld + (size_t)c];
    const int row0 = p.row_off[0] + (p.user_slot == 0 ? uid : iid);
    const int row1 = p.row_off[1] + (p.user_slot == 0 ? iid : uid);
    const f32x4 e0 = load_flat4<TD>(p.tables, (size_t)row0 * DQ + q);
    const f32x4 e1 = load_flat4<TD>(p.tables, (size_t)row1 * DQ + q);
    const float w0 = p.w1 != nullptr ? p.w1[row0] : 0.f;
    const float w1 = p.w1 != nullptr ? p.w1[row1] : 0.f;
    *reinterpret_cast<f32x4*>(X + r * ldx + q * 4) = e0;
    *reinterpret_cast<f32x4*>(X + r * ldx + D + q * 4) = e1;
    const f32x4 s = e0 + e1, qq = e0 * e0 + e1 * e1;
    float a1 = 0.f;
    if (p.w1_mask & 1ull) a1 += w0;
    if (p.w1_mask & 2ull) a1 += w1;
    float t = ((s[0] * s[0] - qq[0]) + (s[1] * s[1] - qq[1])) + ((s[2] * s[2] - qq[2]) + (s[3] * s[3] - qq[3]));
#pragma unroll
    for (int m = 1; m < DQ; m <<= 1) t += __shfl_xor(t, m);     // over the quarters q
    if (q == 0) {
      ys[r] = a1;
      ys[16 + r] = 0.5f * t;
    }
  }
  __syncthreads();
  // ---- the tower, then the 1-unit layer, the logits layer, sigmoid: thread (r, d) of the first 256 ----
  const float* AL = run_tower(p.t, lds, 2 * D, tid);
  if (tid < 256) {
    const int r = tid >> 4, d = tid & 15;
    const float t0 = fmaxf(ys[r] + (p.c0 != nullptr ? p.c0[0] : 0.f), 0.f);
    float z = p.wo[0] * t0 + p.wo[1] * ys[16 + r];
    const int NL = p.t.L == 1 ? p.t.N[0] : (p.t.L == 2 ? p.t.N[1] : p.t.N[2]);
    z += p.wo[2] * fmaxf(head_dot16(AL + r * p.t.lda, p.wd, NL, d) + p.bd[0], 0.f);
    z += p.bo[0];
    if (d == 0 && c0 + r < p.C) p.prob[(size_t)u * (size_t)p.C + (size_t)(c0 + r)] = 1.f / (1.f + expf(-z));
  }
}

template <int TD>
int launch_pair(const PairArgs& p, const int D, const unsigned grid, const size_t lds, hipStream_t stream) {
  switch (D) {
    case 8: return launch_big_lds<predict_pair_rank_k<TD, 8>>(p, grid, PR_T, lds, stream);
    case 16: return launch_big_lds<predict_pair_rank_k<TD, 16>>(p, grid, PR_T, lds, stream);
    default: return launch_big_lds<predict_pair_rank_k<TD, 32>>(p, grid, PR_T, lds, stream);
  }
}

}  // namespace

extern "C" int rsx_predict_pair_rank_supported(int U, int C, int D, int L, const int32_t* widths) {
  return pair_lds_floats(U, C, D, L, widths, nullptr) >= 0 ? 1 : 0;
}

extern "C" int rsx_predict_pair_rank(const rsx_predict_model* m, int user_slot, const int32_t* user_id, const int32_t* item_id,
                                     int item_ld, float* prob, int U, int C, rsx_stream_t stream) {
  if (!m || !user_id || !item_id || !prob || U <= 0 || C <= 0) return RSX_EINVAL;
  if ((user_slot != 0 && user_slot != 1) || (item_ld != 0 && item_ld < C)) return RSX_EINVAL;
  if (m->F != 2 || !tower_model_valid(m)) return RSX_EINVAL;
  if (m->L >= 1 && m->L <= RSX_PREDICT_MAX_LAYERS && (!m->wd || !m->bd)) return RSX_EINVAL;
  PairArgs p;
  const long long fl = pair_lds_floats(U, C, m->D, m->L, m->widths, &p.t);
  if (fl < 0) return RSX_EUNSUPPORTED;
  fill_tower(&p.t, m);
  p.tables = m->tables; p.w1 = m->w1; p.row_off = m->row_off; p.user_id = user_id; p.item_id = item_id;
  p.wd = m->wd; p.bd = m->bd; p.c0 = m->c0; p.wo = m->wo; p.bo = m->bo;
  p.prob = prob;
  p.w1_mask = m->w1_field_mask;
  p.U = U; p.C = C; p.item_ld = item_ld; p.user_slot = user_slot;
  p.tiles = (C + PR_ROWS - 1) / PR_ROWS;
  const unsigned grid = (unsigned)((long long)U * p.tiles);
  const size_t lds = (size_t)fl * sizeof(float);
  return dispatch_table_dtype(m->table_dtype, [&](auto td) {
    return launch_pair<decltype(td)::value>(p, m->D, grid, lds, rsx_s(stream));
  });
}
