// Serialized tf.train.Example records (Criteo-39) -> ids int32 [n, F] on the device: the parse of a serving request as one
// launch in front of the predict kernel (rsx_predict_fm_tower / rsx_predict_dcn), so that `Predictor.predict_examples` ships
// the raw request bytes and the host neither walks the protobuf nor hashes.  The byte-level routines are parse_device.h's
// (shared with the host twin below); this file holds the orchestration:
//
//   one workgroup of ONE wave per example.  The wave copies the record into LDS with aligned 4-byte loads (coalesced), walks
//   the two outer message levels together (every lane reads the same LDS byte: a broadcast read) and hands map entry i of a
//   round to lane i, which decodes the key, finds the first value and hashes it.  Lane t < 40 then owns field `_c<t>` and takes
//   the value of the LAST entry that gave it one (rounds of 64 entries keep wire order); lane s < F finally turns slot s's
//   field into an id.  No atomics; ids and status are written with ordinary stores, the status once per example.
//
// The contract is "decline, never guess": status 0 means ids[r, :] are exactly what rsx_criteo_parse_row (label optional)
// writes; any other status means the row of ids was NOT written and the caller parses the request on the host.
#include <cmath>
#include <cstring>

#include "parse_device.h"
#include "rsx_common.h"

namespace {
constexpr int PX_T = RSX_WAVE;
constexpr int PX_FIELDS = 40;

__global__ __launch_bounds__(PX_T) void parse_examples_k(const uint8_t* __restrict__ buf, const uint32_t buf_bytes,
                                                          const int32_t* __restrict__ offs, const pd_spec sp,
                                                          int32_t* __restrict__ ids, int32_t* __restrict__ status) {
  __shared__ uint32_t stage[RSX_PARSE_MAX_RECORD / 4 + 2];
  __shared__ int32_t e_j[PX_T];
  __shared__ uint64_t e_v[PX_T];
  __shared__ uint64_t f_v[PX_FIELDS];
  __shared__ int32_t f_have[PX_FIELDS];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t a = offs[r], b = offs[r + 1];
  // everything up to the staging loop is uniform over the wave
  int st = RSX_PARSE_OK;
  if (a < 0 || b < a || (uint32_t)b > buf_bytes) st = RSX_PARSE_BAD_OFFSETS;
  else if (b - a > RSX_PARSE_MAX_RECORD) st = RSX_PARSE_TOO_LONG;
  else if (__ballot(lane < sp.F && pd_slot_bad(sp, lane)) != 0ull) st = RSX_PARSE_BAD_SPEC;
  if (st != RSX_PARSE_OK) {
    if (lane == 0) status[r] = st;
    return;
  }
  // the record's bytes [a, b) as the 4-byte words that cover them: the last word ends at most at buf_bytes (a multiple of 4)
  const uint32_t w0 = (uint32_t)a >> 2, nw = (((uint32_t)b + 3u) >> 2) - w0;
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(buf) + w0;
  for (uint32_t w = lane; w < nw; w += PX_T) stage[w] = src[w];
  __syncthreads();
  const uint8_t* rec = reinterpret_cast<const uint8_t*>(stage) + (a & 3);
  const uint32_t n = (uint32_t)(b - a);

  pd_entry_iter it;
  pd_iter_init(it, n);
  bool have = false;          // lane t < 40: field _c<t> has a value
  uint64_t val = 0;
  bool bad = false, more = true;
  while (more && !bad) {
    // up to 64 entries of this round: all lanes walk the same bytes, lane i keeps entry i
    int cnt = 0;
    uint32_t mo = 0, ml = 0;
    while (cnt < PX_T) {
      uint32_t o = 0, l = 0;
      const int rr = pd_next_entry(rec, it, o, l);
      if (rr <= 0) {
        more = false;
        bad = rr < 0;
        break;
      }
      if (cnt == lane) {
        mo = o;
        ml = l;
      }
      ++cnt;
    }
    if (bad) break;
    int j = -1;
    uint64_t v = 0;
    bool mybad = false;
    if (lane < cnt) {
      const int rr = pd_parse_entry(rec, mo, ml, j, v);
      mybad = rr < 0;
      if (rr <= 0) j = -1;
    }
    if (__ballot(mybad) != 0ull) {
      bad = true;
      break;
    }
    e_j[lane] = j;
    e_v[lane] = v;
    __syncthreads();
    if (lane < PX_FIELDS)
      for (int k = 0; k < cnt; ++k)
        if (e_j[k] == lane) {
          have = true;
          val = e_v[k];
        }
    __syncthreads();
  }
  if (!bad && __ballot(lane >= 1 && lane <= 13 && !have) != 0ull) st = RSX_PARSE_MISSING_NUMERIC;
  if (bad) st = RSX_PARSE_MALFORMED;
  if (st == RSX_PARSE_OK) {
    if (lane < PX_FIELDS) {
      f_v[lane] = val;
      f_have[lane] = have ? 1 : 0;
    }
    __syncthreads();
    if (lane < sp.F) {
      const int j = sp.slot_src[lane];
      ids[(size_t)r * sp.F + lane] = pd_slot_id(sp, lane, f_have[j] != 0, f_v[j]);
    }
  }
  if (lane == 0) status[r] = st;
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The checks both entries share (everything that can be seen without reading a buffer).
int check_args(const void* buf, int64_t buf_bytes, const int32_t* offs, int n, const rsx_parse_spec* s, const int32_t* ids,
               const int32_t* status) {
  if (!buf || !offs || !s || !ids || !status || n <= 0) return RSX_EINVAL;
  if (!s->slot_src || !s->slot_rows || !s->thr || !s->thr_off || !s->shift || s->F <= 0) return RSX_EINVAL;
  if (buf_bytes <= 0 || buf_bytes > 0x7ffffffcll || (buf_bytes & 3)) return RSX_EINVAL;
  if (!al4(buf) || !al4(offs) || !al4(ids) || !al4(status)) return RSX_EINVAL;
  if (!rsx_criteo_parse_examples_supported(n, s->F)) return RSX_EUNSUPPORTED;
  return RSX_OK;
}

pd_spec spec_of(const rsx_parse_spec* s) {
  pd_spec sp;
  sp.slot_src = s->slot_src; sp.slot_rows = s->slot_rows; sp.thr = s->thr; sp.thr_off = s->thr_off; sp.shift = s->shift;
  sp.F = s->F; sp.null_hash = s->null_hash;
  return sp;
}
}  // namespace

extern "C" int rsx_criteo_parse_examples_supported(int n, int F) { return (n >= 1 && F >= 1 && F <= 64) ? 1 : 0; }

extern "C" int rsx_criteo_parse_examples(const uint8_t* buf, int64_t buf_bytes, const int32_t* offs, int n,
                                         const rsx_parse_spec* spec_h, int32_t* ids, int32_t* status, rsx_stream_t stream) {
  const int st = check_args(buf, buf_bytes, offs, n, spec_h, ids, status);
  if (st != RSX_OK) return st;
  RSX_LAUNCH(parse_examples_k, dim3(n), dim3(PX_T), 0, rsx_s(stream), buf, (uint32_t)buf_bytes, offs, spec_of(spec_h), ids,
             status);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}

// The host twin: the same routines and the same decisions in a plain loop (host pointers throughout).
extern "C" int rsx_criteo_parse_dev_h(const uint8_t* buf_h, int64_t buf_bytes, const int32_t* offs_h, int n,
                                      const rsx_parse_spec* spec_h, int32_t* ids_h, int32_t* status_h) {
  const int stc = check_args(buf_h, buf_bytes, offs_h, n, spec_h, ids_h, status_h);
  if (stc != RSX_OK) return stc;
  const pd_spec sp = spec_of(spec_h);
  bool bad_spec = false;
  for (int s = 0; s < sp.F; ++s) bad_spec = bad_spec || pd_slot_bad(sp, s);
  for (int r = 0; r < n; ++r) {
    const int32_t a = offs_h[r], b = offs_h[r + 1];
    int st = RSX_PARSE_OK;
    if (a < 0 || b < a || (int64_t)b > buf_bytes) st = RSX_PARSE_BAD_OFFSETS;
    else if (b - a > RSX_PARSE_MAX_RECORD) st = RSX_PARSE_TOO_LONG;
    else if (bad_spec) st = RSX_PARSE_BAD_SPEC;
    if (st == RSX_PARSE_OK) {
      const uint8_t* rec = buf_h + a;
      pd_entry_iter it;
      pd_iter_init(it, (uint32_t)(b - a));
      bool have[PX_FIELDS] = {false};
      uint64_t val[PX_FIELDS] = {0};
      uint32_t o = 0, l = 0;
      int rr;
      while ((rr = pd_next_entry(rec, it, o, l)) > 0) {
        int j = -1;
        uint64_t v = 0;
        const int re = pd_parse_entry(rec, o, l, j, v);
        if (re < 0) { rr = -1; break; }
        if (re > 0) { have[j] = true; val[j] = v; }
      }
      if (rr < 0) st = RSX_PARSE_MALFORMED;
      else
        for (int j = 1; j <= 13; ++j)
          if (!have[j]) st = RSX_PARSE_MISSING_NUMERIC;
      if (st == RSX_PARSE_OK)
        for (int s = 0; s < sp.F; ++s) {
          const int j = sp.slot_src[s];
          ids_h[(size_t)r * sp.F + s] = pd_slot_id(sp, s, have[j], val[j]);
        }
    }
    status_h[r] = st;
  }
  return RSX_OK;
}

extern "C" uint64_t rsx_fingerprint64_dev_h(const uint8_t* s_h, size_t n) {
  return n > 0xffffffffull ? 0 : pd_fp64(s_h, (uint32_t)n);
}

extern "C" int rsx_bucketize_thr_h(const float* x_h, int64_t n, const float* thr_h, int nb, float shift, int32_t* out_h) {
  if (n < 0 || nb < 0 || (n > 0 && (!x_h || !out_h)) || (nb > 0 && !thr_h)) return RSX_EINVAL;
  for (int64_t i = 0; i < n; ++i) out_h[i] = pd_bucket(thr_h, nb, x_h[i] + shift);
  return RSX_OK;
}

// thr_h[k] = the smallest non-negative float v, in bit-pattern order from +0 to +inf, with logf(v) >= boundaries_h[k], found by
// bisection on THIS host's logf and verified per boundary: logf(prev(thr)) < b <= logf(thr).
extern "C" int rsx_log_thresholds_h(const float* boundaries_h, int nb, float* thr_h) {
  if (nb < 0 || (nb > 0 && (!boundaries_h || !thr_h))) return RSX_EINVAL;
  for (int k = 0; k < nb; ++k) {
    const float b = boundaries_h[k];
    if (!std::isfinite(b) || (k > 0 && b < boundaries_h[k - 1])) return RSX_EINVAL;
  }
  auto val = [](uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; };
  for (int k = 0; k < nb; ++k) {
    const float b = boundaries_h[k];
    uint32_t lo = 0, hi = 0x7f800000u;                 // logf(+0) = -inf < b <= +inf = logf(+inf)
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (logf(val(mid)) >= b) hi = mid; else lo = mid;
    }
    if (!(logf(val(hi - 1)) < b) || !(b <= logf(val(hi)))) return RSX_EUNSUPPORTED;
    thr_h[k] = val(hi);
  }
  return RSX_OK;
}
