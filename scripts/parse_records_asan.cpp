// Bounds check of the records half of csrc/parse_device.h on the CPU: reads records (int32 count, then per record int32
// length + bytes; tests/parse_records_util.py's labelled corpora written that way) from the file named on the command line,
// places each record in a heap allocation of exactly its length and runs the label-aware parse and the 64-lane CRC (chunk
// routine and combine step of every virtual lane) over it.  Build with -fsanitize=address,undefined: a read outside
// [rec, rec + n) aborts; the lane CRC is compared with a serial bitwise CRC on the way.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irecsys_amd/csrc \
//       scripts/parse_records_asan.cpp -o parse_records_asan && ./parse_records_asan records.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "parse_device.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  long accepted = 0, malformed = 0, missing = 0, no_label = 0, crc_bad = 0;
  uint64_t digest = 0;
  for (int32_t r = 0; r < count; ++r) {
    int32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    uint8_t* rec = static_cast<uint8_t*>(std::malloc(n ? n : 1)) + (n ? 0 : 1);      // n == 0: one past a 1-byte block
    if (n && std::fread(rec, 1, n, f) != (size_t)n) return 2;
    // the 64-lane CRC against the serial one
    uint32_t serial = 0xffffffffu;
    for (int32_t i = 0; i < n; ++i) serial = pd_crc_byte(serial, rec[i]);
    serial = pd_crc_mask(serial ^ 0xffffffffu);
    uint32_t lanes;
    if (n < 4) {
      lanes = pd_crc_mask(pd_crc_short(rec, (uint32_t)n));
    } else {
      const uint32_t L = ((uint32_t)n + 63u) >> 6, xL = pd_crc_xpow8(L);
      uint32_t c = 0;
      for (int lane = 0; lane < 64; ++lane) c ^= pd_crc_shift(pd_crc_chunk(rec, (uint32_t)n, L, lane), xL, lane);
      lanes = pd_crc_mask(c ^ 0xffffffffu);
    }
    if (lanes != serial) ++crc_bad;
    // the label-aware parse
    pd_entry_iter it;
    pd_iter_init(it, (uint32_t)n);
    bool have[40] = {false};
    uint64_t val[40] = {0};
    uint32_t o = 0, l = 0;
    int rr;
    while ((rr = pd_next_entry(rec, it, o, l)) > 0) {
      int j = -1;
      uint64_t v = 0;
      const int re = pd_parse_entry_label(rec, o, l, j, v);
      if (re < 0) { rr = -1; break; }
      if (re > 0) { have[j] = true; val[j] = v; }
    }
    bool miss = false;
    for (int j = 1; j <= 13; ++j) miss = miss || !have[j];
    if (rr < 0) ++malformed; else if (miss) ++missing; else if (!have[0]) ++no_label; else ++accepted;
    for (int j = 0; j < 40; ++j) digest = digest * 1099511628211ull + (have[j] ? val[j] : 7);
    digest ^= lanes;
    std::free(rec - (n ? 0 : 1));
  }
  std::fclose(f);
  std::printf("records %d accepted %ld malformed %ld missing_numeric %ld missing_label %ld lane_crc_mismatches %ld digest %016llx\n",
              (int)count, accepted, malformed, missing, no_label, crc_bad, (unsigned long long)digest);
  return crc_bad ? 1 : 0;
}
