// Framed TFRecord records (Criteo-39) -> label fp32 and ids int32 [F] of several batches on the device, in the packing the
// Estimator consumes: the parse of the input_fn stream (`criteo_input_fn(device_parse=True)`) as ONE launch per chunk of
// batches, so that the host ships raw shard bytes and neither walks the protobuf, hashes, takes a logf nor computes a
// payload CRC.  The byte-level routines are parse_device.h's (shared with the host twin below); this file holds the
// orchestration, which is parse_examples_k's plus the framing:
//
//   one workgroup of ONE wave per record.  The wave copies the record WITH its framing (12 bytes in front: u64 length, u32
//   masked crc of it; 4 bytes behind: u32 masked crc of the payload) into LDS once, with aligned 4-byte loads.  With
//   verify_crc the 64 lanes take a chunk of the payload each, move the chunk's CRC to its place by a multiplication in GF(2)
//   and xor-reduce over the wave (the header's 8 bytes go the same way).  Then the walk of parse_examples_k: lane i takes
//   map entry i, lane t < 40 owns field `_c<t>` -- lane 0 the label, which is REQUIRED here -- lane s < F writes slot s's id.
//   No atomics; label, ids and status are written with ordinary stores, the status once per record.
//
// The contract is "decline, never guess": status 0 means the label and ids[F] of the record are exactly what
// rsx_criteo_parse_row (label required) writes; any other status means NEITHER was written and the caller parses on the host.
#include "parse_device.h"
#include "rsx_common.h"

namespace {
constexpr int PR_T = RSX_WAVE;
constexpr int PR_FIELDS = 40;
constexpr int PR_FRAME_HEAD = 12, PR_FRAME_TAIL = 4;

// The output description of a launch: record r's batch is r / rows, its row r % rows.
struct pr_out {
  uint8_t* base;
  int32_t rows;
  int64_t stride, ids_off;
};

// The 64-lane masked CRC-32C of rec[0, n) (every lane returns it).  Uniform control flow; rec is the staged record in LDS.
__device__ inline uint32_t crc_wave(const uint8_t* rec, uint32_t n, int lane) {
  if (n < 4u) return pd_crc_mask(pd_crc_short(rec, n));
  const uint32_t L = (n + 63u) >> 6;
  uint32_t c = pd_crc_shift(pd_crc_chunk(rec, n, L, lane), pd_crc_xpow8(L), lane);
  for (int m = 32; m >= 1; m >>= 1) c ^= (uint32_t)__shfl_xor((int)c, m, PR_T);
  return pd_crc_mask(c ^ 0xffffffffu);
}

__global__ __launch_bounds__(PR_T) void parse_records_k(const uint8_t* __restrict__ buf, const uint32_t buf_bytes,
                                                         const int32_t* __restrict__ rec_off,
                                                         const int32_t* __restrict__ rec_len, const pd_spec sp,
                                                         const int verify_crc, const pr_out o,
                                                         int32_t* __restrict__ status) {
  // payload + framing, plus the up to 3 bytes in front of the first and behind the last that their aligned words hold
  __shared__ uint32_t stage[(RSX_PARSE_MAX_RECORD + PR_FRAME_HEAD + PR_FRAME_TAIL) / 4 + 2];
  __shared__ int32_t e_j[PR_T];
  __shared__ uint64_t e_v[PR_T];
  __shared__ uint64_t f_v[PR_FIELDS];
  __shared__ int32_t f_have[PR_FIELDS];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t po = rec_off[r], pl = rec_len[r];
  // everything up to the staging loop is uniform over the wave
  int st = RSX_PARSE_OK;
  if (po < PR_FRAME_HEAD || pl < 0 || (uint64_t)po + (uint64_t)pl + PR_FRAME_TAIL > (uint64_t)buf_bytes) st = RSX_PARSE_BAD_OFFSETS;
  else if (__ballot(lane < sp.F && pd_slot_bad(sp, lane)) != 0ull) st = RSX_PARSE_BAD_SPEC;
  else if (pl > RSX_PARSE_MAX_RECORD) st = RSX_PARSE_TOO_LONG;
  if (st != RSX_PARSE_OK) {
    if (lane == 0) status[r] = st;
    return;                   // the whole wave leaves, in front of the first barrier
  }
  // the bytes [a, b) = framing | payload | framing as the 4-byte words that cover them: the last word ends at most at buf_bytes
  const uint32_t a = (uint32_t)po - PR_FRAME_HEAD, b = (uint32_t)po + (uint32_t)pl + PR_FRAME_TAIL;
  const uint32_t w0 = a >> 2, nw = ((b + 3u) >> 2) - w0;
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(buf) + w0;
  for (uint32_t w = lane; w < nw; w += PR_T) stage[w] = src[w];
  __syncthreads();
  const uint8_t* head = reinterpret_cast<const uint8_t*>(stage) + (a & 3);
  const uint8_t* rec = head + PR_FRAME_HEAD;
  const uint32_t n = (uint32_t)pl;

  if (verify_crc) {           // uniform: every lane holds the same three answers
    bool ok = pd_ld32(head) == n && pd_ld32(head + 4) == 0u;
    ok = ok && crc_wave(head, 8u, lane) == pd_ld32(head + 8);
    ok = ok && crc_wave(rec, n, lane) == pd_ld32(rec + n);
    if (!ok) {
      if (lane == 0) status[r] = RSX_PARSE_CRC;
      return;
    }
  }

  pd_entry_iter it;
  pd_iter_init(it, n);
  bool have = false;          // lane t < 40: field _c<t> has a value
  uint64_t val = 0;
  bool bad = false, more = true;
  while (more && !bad) {
    // up to 64 entries of this round: all lanes walk the same bytes, lane i keeps entry i
    int cnt = 0;
    uint32_t mo = 0, ml = 0;
    while (cnt < PR_T) {
      uint32_t eo = 0, el = 0;
      const int rr = pd_next_entry(rec, it, eo, el);
      if (rr <= 0) {
        more = false;
        bad = rr < 0;
        break;
      }
      if (cnt == lane) {
        mo = eo;
        ml = el;
      }
      ++cnt;
    }
    if (bad) break;
    int j = -1;
    uint64_t v = 0;
    bool mybad = false;
    if (lane < cnt) {
      const int rr = pd_parse_entry_label(rec, mo, ml, j, v);
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
    if (lane < PR_FIELDS)
      for (int k = 0; k < cnt; ++k)
        if (e_j[k] == lane) {
          have = true;
          val = e_v[k];
        }
    __syncthreads();
  }
  if (!bad) {
    if (__ballot(lane >= 1 && lane <= 13 && !have) != 0ull) st = RSX_PARSE_MISSING_NUMERIC;
    else if (__ballot(lane == 0 && !have) != 0ull) st = RSX_PARSE_MISSING_LABEL;
  }
  if (bad) st = RSX_PARSE_MALFORMED;
  if (st == RSX_PARSE_OK) {
    if (lane < PR_FIELDS) {
      f_v[lane] = val;
      f_have[lane] = have ? 1 : 0;
    }
    __syncthreads();
    uint8_t* batch = o.base + (size_t)(r / o.rows) * (size_t)o.stride;
    const size_t row = (size_t)(r % o.rows);
    if (lane == 0) reinterpret_cast<uint32_t*>(batch)[row] = (uint32_t)val;         // the label's bit pattern
    if (lane < sp.F) {
      const int j = sp.slot_src[lane];
      reinterpret_cast<int32_t*>(batch + o.ids_off)[row * sp.F + lane] = pd_slot_id(sp, lane, f_have[j] != 0, f_v[j]);
    }
  }
  if (lane == 0) status[r] = st;
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The checks both entries share (everything that can be seen without reading a buffer).
int check_args(const void* buf, int64_t buf_bytes, const int32_t* rec_off, const int32_t* rec_len, int n, const rsx_parse_spec* s,
               const void* out, int rows_per_batch, int64_t batch_stride, int64_t ids_off, const int32_t* status) {
  if (!buf || !rec_off || !rec_len || !s || !out || !status || n <= 0 || rows_per_batch <= 0) return RSX_EINVAL;
  if (!s->slot_src || !s->slot_rows || !s->thr || !s->thr_off || !s->shift || s->F <= 0) return RSX_EINVAL;
  if (buf_bytes <= 0 || buf_bytes > 0x7ffffffcll || (buf_bytes & 3)) return RSX_EINVAL;
  if (!al4(buf) || !al4(rec_off) || !al4(rec_len) || !al4(out) || !al4(status)) return RSX_EINVAL;
  if ((batch_stride & 3) || (ids_off & 3) || ids_off < 4ll * rows_per_batch) return RSX_EINVAL;
  if (!rsx_criteo_parse_records_supported(n, s->F)) return RSX_EUNSUPPORTED;
  if (batch_stride < ids_off + 4ll * s->F * rows_per_batch) return RSX_EINVAL;
  return RSX_OK;
}

pd_spec spec_of(const rsx_parse_spec* s) {
  pd_spec sp;
  sp.slot_src = s->slot_src; sp.slot_rows = s->slot_rows; sp.thr = s->thr; sp.thr_off = s->thr_off; sp.shift = s->shift;
  sp.F = s->F; sp.null_hash = s->null_hash;
  return sp;
}

// The twin's CRC: the kernel's routines over 64 VIRTUAL lanes (chunk, shift, xor), not a serial CRC.
uint32_t crc_lanes_h(const uint8_t* rec, uint32_t n) {
  if (n < 4u) return pd_crc_mask(pd_crc_short(rec, n));
  const uint32_t L = (n + 63u) >> 6, xL = pd_crc_xpow8(L);
  uint32_t c = 0;
  for (int lane = 0; lane < PR_T; ++lane) c ^= pd_crc_shift(pd_crc_chunk(rec, n, L, lane), xL, lane);
  return pd_crc_mask(c ^ 0xffffffffu);
}
}  // namespace

extern "C" int rsx_criteo_parse_records_supported(int n, int F) { return (n >= 1 && F >= 1 && F <= 64) ? 1 : 0; }

extern "C" int rsx_criteo_parse_records(const uint8_t* buf, int64_t buf_bytes, const int32_t* rec_off, const int32_t* rec_len,
                                        int n, const rsx_parse_spec* spec_h, int verify_crc, void* out, int rows_per_batch,
                                        int64_t batch_stride, int64_t ids_off, int32_t* status, rsx_stream_t stream) {
  const int st = check_args(buf, buf_bytes, rec_off, rec_len, n, spec_h, out, rows_per_batch, batch_stride, ids_off, status);
  if (st != RSX_OK) return st;
  pr_out o;
  o.base = static_cast<uint8_t*>(out); o.rows = rows_per_batch; o.stride = batch_stride; o.ids_off = ids_off;
  RSX_LAUNCH(parse_records_k, dim3(n), dim3(PR_T), 0, rsx_s(stream), buf, (uint32_t)buf_bytes, rec_off, rec_len,
             spec_of(spec_h), verify_crc ? 1 : 0, o, status);
  RSX_CHECK_LAUNCH();
  return RSX_OK;
}

// The host twin: the same routines and the same decisions in a plain loop (host pointers throughout).
extern "C" int rsx_criteo_parse_records_dev_h(const uint8_t* buf_h, int64_t buf_bytes, const int32_t* rec_off_h,
                                              const int32_t* rec_len_h, int n, const rsx_parse_spec* spec_h, int verify_crc,
                                              void* out_h, int rows_per_batch, int64_t batch_stride, int64_t ids_off,
                                              int32_t* status_h) {
  const int stc = check_args(buf_h, buf_bytes, rec_off_h, rec_len_h, n, spec_h, out_h, rows_per_batch, batch_stride, ids_off,
                             status_h);
  if (stc != RSX_OK) return stc;
  const pd_spec sp = spec_of(spec_h);
  bool bad_spec = false;
  for (int s = 0; s < sp.F; ++s) bad_spec = bad_spec || pd_slot_bad(sp, s);
  for (int r = 0; r < n; ++r) {
    const int32_t po = rec_off_h[r], pl = rec_len_h[r];
    int st = RSX_PARSE_OK;
    if (po < PR_FRAME_HEAD || pl < 0 || (int64_t)po + pl + PR_FRAME_TAIL > buf_bytes) st = RSX_PARSE_BAD_OFFSETS;
    else if (bad_spec) st = RSX_PARSE_BAD_SPEC;
    else if (pl > RSX_PARSE_MAX_RECORD) st = RSX_PARSE_TOO_LONG;
    const uint8_t* rec = st == RSX_PARSE_OK ? buf_h + po : buf_h;
    const uint8_t* head = st == RSX_PARSE_OK ? rec - PR_FRAME_HEAD : buf_h;
    const uint32_t len = (uint32_t)pl;
    if (st == RSX_PARSE_OK && verify_crc) {
      bool ok = pd_ld32(head) == len && pd_ld32(head + 4) == 0u;
      ok = ok && crc_lanes_h(head, 8u) == pd_ld32(head + 8);
      ok = ok && crc_lanes_h(rec, len) == pd_ld32(rec + len);
      if (!ok) st = RSX_PARSE_CRC;
    }
    if (st == RSX_PARSE_OK) {
      pd_entry_iter it;
      pd_iter_init(it, len);
      bool have[PR_FIELDS] = {false};
      uint64_t val[PR_FIELDS] = {0};
      uint32_t eo = 0, el = 0;
      int rr;
      while ((rr = pd_next_entry(rec, it, eo, el)) > 0) {
        int j = -1;
        uint64_t v = 0;
        const int re = pd_parse_entry_label(rec, eo, el, j, v);
        if (re < 0) { rr = -1; break; }
        if (re > 0) { have[j] = true; val[j] = v; }
      }
      if (rr < 0) st = RSX_PARSE_MALFORMED;
      else {
        bool numeric = true;
        for (int j = 1; j <= 13; ++j) numeric = numeric && have[j];
        if (!numeric) st = RSX_PARSE_MISSING_NUMERIC;
        else if (!have[0]) st = RSX_PARSE_MISSING_LABEL;
      }
      if (st == RSX_PARSE_OK) {
        uint8_t* batch = static_cast<uint8_t*>(out_h) + (size_t)(r / rows_per_batch) * (size_t)batch_stride;
        const size_t row = (size_t)(r % rows_per_batch);
        reinterpret_cast<uint32_t*>(batch)[row] = (uint32_t)val[0];
        int32_t* ids = reinterpret_cast<int32_t*>(batch + ids_off) + row * sp.F;
        for (int s = 0; s < sp.F; ++s) {
          const int j = sp.slot_src[s];
          ids[s] = pd_slot_id(sp, s, have[j], val[j]);
        }
      }
    }
    status_h[r] = st;
  }
  return RSX_OK;
}

extern "C" uint32_t rsx_masked_crc32c_dev_h(const uint8_t* p_h, size_t n) {
  return (n > 0x7fffffffull || (n && !p_h)) ? 0 : crc_lanes_h(p_h, (uint32_t)n);
}

extern "C" int rsx_thread_capture_relaxed_h(void) {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  return hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess ? RSX_OK : RSX_ELAUNCH;
}
