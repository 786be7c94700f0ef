// Bounds check of csrc/parse_device.h on the CPU: reads records (int32 count, then per record int32 length + bytes) from the
// file named on the command line, places each record at the very END of its own heap allocation and runs every byte-level
// routine of the device parse over it.  Build with -fsanitize=address,undefined: a read outside [rec, rec + n) aborts.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irecsys_amd/csrc \
//       scripts/parse_device_asan.cpp -o parse_device_asan && ./parse_device_asan records.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "parse_device.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  long accepted = 0, malformed = 0, missing = 0;
  uint64_t digest = 0;
  for (int32_t r = 0; r < count; ++r) {
    int32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    uint8_t* rec = static_cast<uint8_t*>(std::malloc(n ? n : 1)) + (n ? 0 : 1);      // n == 0: one past a 1-byte block
    if (n && std::fread(rec, 1, n, f) != (size_t)n) return 2;
    pd_entry_iter it;
    pd_iter_init(it, (uint32_t)n);
    bool have[40] = {false};
    uint64_t val[40] = {0};
    uint32_t o = 0, l = 0;
    int rr;
    while ((rr = pd_next_entry(rec, it, o, l)) > 0) {
      int j = -1;
      uint64_t v = 0;
      const int re = pd_parse_entry(rec, o, l, j, v);
      if (re < 0) { rr = -1; break; }
      if (re > 0) { have[j] = true; val[j] = v; }
    }
    bool miss = false;
    for (int j = 1; j <= 13; ++j) miss = miss || !have[j];
    if (rr < 0) ++malformed; else if (miss) ++missing; else ++accepted;
    for (int j = 1; j < 40; ++j) digest = digest * 1099511628211ull + (have[j] ? val[j] : 7);
    digest ^= pd_fp64(rec, (uint32_t)n);                                             // the whole record through the hash too
    std::free(rec - (n ? 0 : 1));
  }
  std::fclose(f);
  std::printf("records %d accepted %ld malformed %ld missing_numeric %ld digest %016llx\n", (int)count, accepted, malformed,
              missing, (unsigned long long)digest);
  return 0;
}
