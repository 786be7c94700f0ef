// Byte-level routines of the device parse of serialized tf.train.Example records (Criteo-39 schema): the same functions run
// in the kernel of parse_examples.hip (over a record staged in LDS) and in its host twin rsx_criteo_parse_dev_h (a plain
// loop on the CPU, what the CPU tests and the sanitizer program exercise).
//
// They restate rsx_criteo_parse_row (tfrecord_ingest.cpp, label_optional = true) over OFFSETS into one record instead of
// pointers: rd_varint / next_field / for_each_feature / feat_first_float / feat_first_bytes / key_cN / fp64 line by line,
// so that a record the host parser accepts is accepted here with the same ids, and one it refuses is declined.
//
// Bounds: every routine takes (rec, ...) with offsets p <= e <= n of the record [rec, rec + n) and reads rec[i] only for
// p <= i < e.  A length read from the wire is compared, as a 64-bit number, with the bytes that are left BEFORE it is added
// to anything; offsets are uint32 and never exceed n, so no sum wraps.
#pragma once
#include <stdint.h>

#include "rsx.h"

#if defined(__HIPCC__)
#define PD_FN __host__ __device__ inline
#else
#define PD_FN inline
#endif

// ---- bounded varint / field reader ------------------------------------------------------------------------------------------
// At most 10 bytes, like the host: the 10th byte's high bits fall off the 64-bit value (over-long varints are accepted).
PD_FN bool pd_varint(const uint8_t* rec, uint32_t& p, uint32_t e, uint64_t& v) {
  v = 0;
  for (int s = 0; s < 64 && p < e; s += 7) {
    const uint8_t b = rec[p++];
    v |= (uint64_t)(b & 0x7f) << s;
    if (!(b & 0x80)) return true;
  }
  return false;
}

// Next field of the message [p, e): 1 = a field (its payload [voff, voff + vlen): the bytes of wire type 2, the 4 / 8 bytes of
// wire types 5 / 1, nothing for a varint), 0 = end of the message, -1 = malformed (a truncated varint, a length past the
// end of the parent, wire types 3 / 4 / 6 / 7).
PD_FN int pd_next_field(const uint8_t* rec, uint32_t& p, uint32_t e, uint32_t& fno, uint32_t& wt, uint32_t& voff,
                        uint32_t& vlen) {
  if (p >= e) return 0;
  uint64_t tag;
  if (!pd_varint(rec, p, e, tag)) return -1;
  fno = (uint32_t)(tag >> 3);
  wt = (uint32_t)(tag & 7);
  if (wt == 2) {
    uint64_t len;
    if (!pd_varint(rec, p, e, len) || len > (uint64_t)(e - p)) return -1;
    voff = p;
    vlen = (uint32_t)len;
    p += (uint32_t)len;
  } else if (wt == 0) {
    uint64_t num;
    if (!pd_varint(rec, p, e, num)) return -1;
    voff = p;
    vlen = 0;
  } else if (wt == 5) {
    if (e - p < 4) return -1;
    voff = p;
    vlen = 4;
    p += 4;
  } else if (wt == 1) {
    if (e - p < 8) return -1;
    voff = p;
    vlen = 8;
    p += 8;
  } else {
    return -1;
  }
  return 1;
}

// ---- map-entry scanner ------------------------------------------------------------------------------------------------------
// Walks Example.features (field 1, repeatable) and, inside each, Features.feature (field 1, the map entries), in wire order.
struct pd_entry_iter {
  uint32_t p, e;      // cursor of the Example message
  uint32_t q, qe;     // cursor of the Features message that is open (q == qe: none)
};
PD_FN void pd_iter_init(pd_entry_iter& it, uint32_t n) {
  it.p = 0;
  it.e = n;
  it.q = 0;
  it.qe = 0;
}
// 1 = the next map entry is [off, off + len), 0 = the record is finished and well formed at these two levels, -1 = malformed.
PD_FN int pd_next_entry(const uint8_t* rec, pd_entry_iter& it, uint32_t& off, uint32_t& len) {
  uint32_t fno = 0, wt = 0, vo = 0, vl = 0;
  for (;;) {
    while (it.q < it.qe) {
      if (pd_next_field(rec, it.q, it.qe, fno, wt, vo, vl) < 0) return -1;
      if (fno == 1 && wt == 2) {
        off = vo;
        len = vl;
        return 1;
      }
    }
    const int r = pd_next_field(rec, it.p, it.e, fno, wt, vo, vl);
    if (r <= 0) return r;
    if (fno == 1 && wt == 2) {
      it.q = vo;
      it.qe = vo + vl;
    }
  }
}

// ---- key "_c0" .. "_c39" -> 0 .. 39, anything else -1 -------------------------------------------------------------------------
PD_FN int pd_key_cN(const uint8_t* rec, uint32_t off, uint32_t len) {
  if (len < 3 || len > 4 || rec[off] != '_' || rec[off + 1] != 'c') return -1;
  int v = 0;
  for (uint32_t i = 2; i < len; ++i) {
    const uint8_t c = rec[off + i];
    if (c < '0' || c > '9') return -1;
    v = v * 10 + (c - '0');
  }
  return v <= 39 ? v : -1;
}

PD_FN uint32_t pd_ld32(const uint8_t* s) {
  return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
}
PD_FN uint64_t pd_ld64(const uint8_t* s) { return (uint64_t)pd_ld32(s) | ((uint64_t)pd_ld32(s + 4) << 32); }

// ---- Feature [off, off + len) -> the first float of its float_list (packed: the first 4 bytes; unpacked: wire type 5) --------
// Malformed bytes inside a Feature end the search without a value; they are no error of the record (as on the host).
PD_FN bool pd_first_float(const uint8_t* rec, uint32_t off, uint32_t len, uint32_t& bits) {
  uint32_t p = off, fno = 0, wt = 0, vo = 0, vl = 0;
  const uint32_t e = off + len;
  while (pd_next_field(rec, p, e, fno, wt, vo, vl) > 0) {
    if (fno != 2 || wt != 2) continue;
    uint32_t q = vo, xo = 0, xl = 0;
    const uint32_t qe = vo + vl;
    while (pd_next_field(rec, q, qe, fno, wt, xo, xl) > 0) {
      if (fno != 1) continue;
      if ((wt == 2 && xl >= 4) || wt == 5) {
        bits = pd_ld32(rec + xo);
        return true;
      }
    }
  }
  return false;
}
// ---- Feature -> the first value of its bytes_list (length 0 is a value) ---------------------------------------------------
PD_FN bool pd_first_bytes(const uint8_t* rec, uint32_t off, uint32_t len, uint32_t& so, uint32_t& sl) {
  uint32_t p = off, fno = 0, wt = 0, vo = 0, vl = 0;
  const uint32_t e = off + len;
  while (pd_next_field(rec, p, e, fno, wt, vo, vl) > 0) {
    if (fno != 1 || wt != 2) continue;
    uint32_t q = vo, xo = 0, xl = 0;
    const uint32_t qe = vo + vl;
    while (pd_next_field(rec, q, qe, fno, wt, xo, xl) > 0)
      if (fno == 1 && wt == 2) {
        so = xo;
        sl = xl;
        return true;
      }
  }
  return false;
}

// ---- FarmHash Fingerprint64 (farmhashna::Hash64; host_ingest.cpp fp64, all four length branches), bytes [s, s + n) ----------
PD_FN uint64_t pd_rot(uint64_t v, int s) { return s == 0 ? v : (v >> s) | (v << (64 - s)); }
PD_FN uint64_t pd_smix(uint64_t v) { return v ^ (v >> 47); }
PD_FN uint64_t pd_h16(uint64_t u, uint64_t v, uint64_t mul) {
  uint64_t a = (u ^ v) * mul;
  a ^= a >> 47;
  uint64_t b = (v ^ a) * mul;
  b ^= b >> 47;
  return b * mul;
}
PD_FN void pd_weak32(const uint8_t* s, uint64_t a, uint64_t b, uint64_t& ra, uint64_t& rb) {
  const uint64_t w = pd_ld64(s), x = pd_ld64(s + 8), y = pd_ld64(s + 16), z = pd_ld64(s + 24);
  a += w;
  b = pd_rot(b + a + z, 21);
  const uint64_t c = a;
  a += x;
  a += y;
  b += pd_rot(a, 44);
  ra = a + z;
  rb = b + c;
}
PD_FN uint64_t pd_fp64(const uint8_t* s, uint32_t n32) {
  const uint64_t k0 = 0xc3a5c85c97cb3127ULL, k1 = 0xb492b66fbe98f273ULL, k2 = 0x9ae16a3b2f90404fULL;
  const uint64_t n = n32;
  if (n <= 16) {
    if (n >= 8) {
      const uint64_t mul = k2 + n * 2, a = pd_ld64(s) + k2, b = pd_ld64(s + n - 8);
      return pd_h16(pd_rot(b, 37) * mul + a, (pd_rot(a, 25) + b) * mul, mul);
    }
    if (n >= 4) {
      const uint64_t mul = k2 + n * 2, a = pd_ld32(s);
      return pd_h16(n + (a << 3), pd_ld32(s + n - 4), mul);
    }
    if (n > 0) {
      const uint32_t y = (uint32_t)s[0] + ((uint32_t)s[n >> 1] << 8), z = (uint32_t)n + ((uint32_t)s[n - 1] << 2);
      return pd_smix(y * k2 ^ z * k0) * k2;
    }
    return k2;
  }
  if (n <= 32) {
    const uint64_t mul = k2 + n * 2, a = pd_ld64(s) * k1, b = pd_ld64(s + 8), c = pd_ld64(s + n - 8) * mul,
                   d = pd_ld64(s + n - 16) * k2;
    return pd_h16(pd_rot(a + b, 43) + pd_rot(c, 30) + d, a + pd_rot(b + k2, 18) + c, mul);
  }
  if (n <= 64) {
    const uint64_t mul = k2 + n * 2, a = pd_ld64(s) * k2, b = pd_ld64(s + 8), c = pd_ld64(s + n - 8) * mul,
                   d = pd_ld64(s + n - 16) * k2;
    const uint64_t y = pd_rot(a + b, 43) + pd_rot(c, 30) + d, z = pd_h16(y, a + pd_rot(b + k2, 18) + c, mul);
    const uint64_t e = pd_ld64(s + 16) * mul, f = pd_ld64(s + 24), g = (y + pd_ld64(s + n - 32)) * mul,
                   h = (z + pd_ld64(s + n - 24)) * mul;
    return pd_h16(pd_rot(e + f, 43) + pd_rot(g, 30) + h, e + pd_rot(f + a, 18) + g, mul);
  }
  const uint64_t seed = 81;
  uint64_t x = seed, y = seed * k1 + 113, z = pd_smix(y * k2 + 113) * k2;
  uint64_t va = 0, vb = 0, wa = 0, wb = 0;
  x = x * k2 + pd_ld64(s);
  const uint8_t* end = s + ((n - 1) / 64) * 64;
  const uint8_t* last64 = end + ((n - 1) & 63) - 63;      // == s + n - 64 >= s
  do {
    x = pd_rot(x + y + va + pd_ld64(s + 8), 37) * k1;
    y = pd_rot(y + vb + pd_ld64(s + 48), 42) * k1;
    x ^= wb;
    y += va + pd_ld64(s + 40);
    z = pd_rot(z + wa, 33) * k1;
    pd_weak32(s, vb * k1, x + wa, va, vb);
    pd_weak32(s + 32, z + wb, y + pd_ld64(s + 16), wa, wb);
    const uint64_t t = z;
    z = x;
    x = t;
    s += 64;
  } while (s != end);
  const uint64_t mul = k1 + ((z & 0xff) << 1);
  s = last64;
  wa += (n - 1) & 63;
  va += wa;
  wa += va;
  x = pd_rot(x + y + va + pd_ld64(s + 8), 37) * mul;
  y = pd_rot(y + vb + pd_ld64(s + 48), 42) * mul;
  x ^= wb * 9;
  y += va * 9 + pd_ld64(s + 40);
  z = pd_rot(z + wa, 33) * mul;
  pd_weak32(s, vb * mul, x + wa, va, vb);
  pd_weak32(s + 32, z + wb, y + pd_ld64(s + 16), wa, wb);
  const uint64_t t = z;
  z = x;
  x = t;
  return pd_h16(pd_h16(va, wa, mul) + pd_smix(y) * k0 + z, pd_h16(vb, wb, mul) + x, mul);
}

// ---- one map entry [off, off + len) ---------------------------------------------------------------------------------------
// 1 = the entry gives field j (1 .. 39) a value: the float's bit pattern (j <= 13) or Fingerprint64 of the bytes (j >= 14);
// 0 = it gives none (no key, a key that is no _c1 .. _c39, no Feature, a Feature without a first value); -1 = malformed.
// (`_c0`, the label, is optional and unused in a serving request: it gives no value here.)
PD_FN int pd_parse_entry(const uint8_t* rec, uint32_t off, uint32_t len, int& j, uint64_t& bits) {
  uint32_t p = off, fno = 0, wt = 0, vo = 0, vl = 0;
  const uint32_t e = off + len;
  bool hk = false, hf = false;
  uint32_t ko = 0, kl = 0, fo = 0, fl = 0;
  int r;
  while ((r = pd_next_field(rec, p, e, fno, wt, vo, vl)) > 0) {
    if (fno == 1 && wt == 2) {
      hk = true;
      ko = vo;
      kl = vl;
    } else if (fno == 2 && wt == 2) {
      hf = true;
      fo = vo;
      fl = vl;
    }
  }
  if (r < 0) return -1;
  if (!hk) return 0;
  j = pd_key_cN(rec, ko, kl);
  if (j <= 0 || !hf) return 0;
  if (j <= 13) {
    uint32_t b;
    if (!pd_first_float(rec, fo, fl, b)) return 0;
    bits = b;
    return 1;
  }
  uint32_t so, sl;
  if (!pd_first_bytes(rec, fo, fl, so, sl)) return 0;
  bits = pd_fp64(rec + so, sl);
  return 1;
}

// ---- threshold bucketize: #boundaries <= logf(v) without a logf -------------------------------------------------------------
// thr[k] is the smallest non-negative float whose host logf reaches boundary k (rsx_log_thresholds_h), non-decreasing.
PD_FN int32_t pd_bucket(const float* thr, int nb, float v) {
  if (v != v || v < 0.f) return nb;                    // logf of a NaN or a negative number is NaN -> nb
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

PD_FN float pd_bits_float(uint32_t u) {
  union { uint32_t u; float f; } c;
  c.u = u;
  return c.f;
}

// What the kernel and the host twin need of rsx_parse_spec (the pointers by value).
struct pd_spec {
  const int32_t* slot_src;
  const int32_t* slot_rows;
  const float* thr;
  const int32_t* thr_off;
  const float* shift;
  int32_t F;
  uint64_t null_hash;
};
// A slot the parser cannot serve: a source field outside _c1 .. _c39, a categorical slot without rows, threshold offsets that
// go backwards.  (Checked per launch on the device: the spec lives in device memory the C entry cannot read.)
PD_FN bool pd_slot_bad(const pd_spec& sp, int s) {
  const int j = sp.slot_src[s];
  if (j < 1 || j > 39) return true;
  if (j >= 14) return sp.slot_rows[s] <= 0;
  return sp.thr_off[s] < 0 || sp.thr_off[s + 1] < sp.thr_off[s];
}
// The id of slot s, given its source field's value (bits as pd_parse_entry returns them; have: the field had a value).
PD_FN int32_t pd_slot_id(const pd_spec& sp, int s, bool have, uint64_t bits) {
  const int j = sp.slot_src[s];
  if (j <= 13) {
    const float v = pd_bits_float((uint32_t)bits) + sp.shift[j - 1];          // one IEEE add, as on the host
    return pd_bucket(sp.thr + sp.thr_off[s], sp.thr_off[s + 1] - sp.thr_off[s], v);
  }
  return (int32_t)((have ? bits : sp.null_hash) % (uint64_t)sp.slot_rows[s]);
}

// ===== TFRecord records of the input_fn stream (parse_records.hip and its host twin rsx_criteo_parse_records_dev_h) ==========

// ---- one map entry, label aware ---------------------------------------------------------------------------------------------
// pd_parse_entry with `_c0` counted: 1 with j == 0 gives the bit pattern of the label's first float (packed or unpacked, through
// pd_first_float, like `_c1` .. `_c13`); everything else as pd_parse_entry.  The training stream REQUIRES the label (the host
// reader answers RSX_EDATA for a record without it), so the caller declines a record whose field 0 got no value.
PD_FN int pd_parse_entry_label(const uint8_t* rec, uint32_t off, uint32_t len, int& j, uint64_t& bits) {
  uint32_t p = off, fno = 0, wt = 0, vo = 0, vl = 0;
  const uint32_t e = off + len;
  bool hk = false, hf = false;
  uint32_t ko = 0, kl = 0, fo = 0, fl = 0;
  int r;
  while ((r = pd_next_field(rec, p, e, fno, wt, vo, vl)) > 0) {
    if (fno == 1 && wt == 2) {
      hk = true;
      ko = vo;
      kl = vl;
    } else if (fno == 2 && wt == 2) {
      hf = true;
      fo = vo;
      fl = vl;
    }
  }
  if (r < 0) return -1;
  if (!hk) return 0;
  j = pd_key_cN(rec, ko, kl);
  if (j < 0 || !hf) return 0;
  if (j <= 13) {
    uint32_t b;
    if (!pd_first_float(rec, fo, fl, b)) return 0;
    bits = b;
    return 1;
  }
  uint32_t so, sl;
  if (!pd_first_bytes(rec, fo, fl, so, sl)) return 0;
  bits = pd_fp64(rec + so, sl);
  return 1;
}

// ---- masked CRC-32C of the TFRecord framing, computed by 64 lanes -------------------------------------------------------------
// CRC-32C (Castagnoli, reflected, polynomial 0x82F63B78), as rsx_crc32c_h: register 0xFFFFFFFF at the start, complemented at the
// end.  A value is a polynomial over GF(2) of degree < 32 whose coefficient of x^k is bit 31 - k (x^0 = 0x80000000).
//
// With a ZERO start register the CRC is linear in the message: crc0(A || B) = crc0(A) * x^(8|B|) mod P  ^  crc0(B), and zero
// bytes in front of a message do not change it.  The start register 0xFFFFFFFF is the same as complementing the first 4
// message bytes (n >= 4).  So the message, right-aligned into 64 chunks of L = ceil(n / 64) bytes (the first chunks are the
// zero bytes in front), is split over 64 lanes: lane i takes chunk i with the bitwise byte step (pd_crc_chunk), multiplies its
// value by x^(8 L (63 - i)) (pd_crc_shift: the six squarings of x^(8L) are the same in every lane, at most six multiplies
// are the lane's own) and the 64 values are xor-ed.  No table: 8 shift-and-xor steps per byte, 32 per multiply.
#define PD_CRC_POLY 0x82F63B78u
PD_FN uint32_t pd_crc_byte(uint32_t c, uint32_t b) {
  c ^= b;
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (PD_CRC_POLY & (0u - (c & 1u)));
  return c;
}
// a * b mod P: a 32-step carry-less multiply
PD_FN uint32_t pd_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; ++k) {
    p ^= b & (0u - ((a >> (31 - k)) & 1u));
    b = (b >> 1) ^ (PD_CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}
// x^(8L) mod P, L >= 1 (square and multiply over the bits of L; the same in every lane)
PD_FN uint32_t pd_crc_xpow8(uint32_t L) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;          // x^0, x^8
  for (; L; L >>= 1) {
    if (L & 1u) r = pd_crc_mul(r, sq);
    sq = pd_crc_mul(sq, sq);
  }
  return r;
}
// Chunk routine of lane `lane` (0 .. 63): the zero-start CRC of bytes [lane * L, (lane + 1) * L) of the right-aligned message
// (64 * L - n zero bytes, then rec[0, n) with its first 4 bytes complemented).  n >= 4, L = ceil(n / 64); reads rec[i], i < n only.
PD_FN uint32_t pd_crc_chunk(const uint8_t* rec, uint32_t n, uint32_t L, int lane) {
  const uint32_t pad = 64u * L - n;                     // < 64
  const uint32_t v0 = (uint32_t)lane * L, v1 = v0 + L;
  uint32_t c = 0;
  for (uint32_t v = v0 < pad ? pad : v0; v < v1; ++v) {
    const uint32_t i = v - pad;
    c = pd_crc_byte(c, (uint32_t)rec[i] ^ (i < 4u ? 0xffu : 0u));
  }
  return c;
}
// Combine step of lane `lane`: c * x^(8 L (63 - lane)) mod P, given xL = x^(8L) -- the chunk's value moved in front of the
// 63 - lane chunks behind it.  The xor of the 64 results is the zero-start CRC of the whole right-aligned message.
PD_FN uint32_t pd_crc_shift(uint32_t c, uint32_t xL, int lane) {
  const uint32_t e = 63u - (uint32_t)lane;
  uint32_t sq = xL;
  for (int k = 0; k < 6; ++k) {
    if ((e >> k) & 1u) c = pd_crc_mul(c, sq);
    sq = pd_crc_mul(sq, sq);
  }
  return c;
}
// Messages shorter than 4 bytes (the start register does not fit into them): the plain serial CRC.
PD_FN uint32_t pd_crc_short(const uint8_t* rec, uint32_t n) {
  uint32_t c = 0xffffffffu;
  for (uint32_t i = 0; i < n; ++i) c = pd_crc_byte(c, rec[i]);
  return c ^ 0xffffffffu;
}
// TFRecord's mask of a CRC (rsx_masked_crc32c_h)
PD_FN uint32_t pd_crc_mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }
