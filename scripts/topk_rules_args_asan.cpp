// Host-side check of csrc/topk_rules.hip on the CPU, no device needed: the LDS plan (rsx_topk_rows_rules_supported) over a grid
// that includes every boundary and absurd sizes, and every refusal of rsx_topk_rows_rules -- all of which return before any HIP
// call.  Build the host code with a sanitizer: an overflow in the plan's arithmetic or a read through a refused pointer aborts.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       -Iinclude -Irecsys_amd/csrc recsys_amd/csrc/topk_rules.hip scripts/topk_rules_args_asan.cpp -o topk_rules_args_asan \
//       && ./topk_rules_args_asan
#include <climits>
#include <cstdint>
#include <cstdio>

#include "rsx.h"

static int fails = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } \
  } while (0)

// the plan restated: the envelope of rsx_topk_rows_excl, m in [0, 16], and with m > 0 the LDS bytes of include/rsx.h
static int expect_supported(long long n, long long k, long long E, long long G, long long m) {
  if (n < 1 || k < 1 || k > 1024 || n + k > 16384 || E < 0 || E > 256 || G < 0 || m < 0 || m > 16) return 0;
  if (m == 0) return 1;
  if (G < 1 || G > 65535) return 0;
  return 10 * (n + k) + 16 * k + 2080 + 16 * G <= 163840 ? 1 : 0;
}

int main() {
  const int ns[] = {INT_MIN, -1, 0, 1, 16, 1000, 4096, 12230, 12231, 13254, 15360, 15361, 16383, 16384, 16385, INT_MAX};
  const int ks[] = {INT_MIN, -1, 0, 1, 8, 100, 1024, 1025, INT_MAX};
  const int Es[] = {INT_MIN, -1, 0, 4, 256, 257, INT_MAX};
  const int Gs[] = {INT_MIN, -1, 0, 1, 3, 802, 8000, 10240, 65535, 65536, INT_MAX};
  const int ms[] = {INT_MIN, -1, 0, 1, 2, 16, 17, INT_MAX};
  long checked = 0;
  for (int n : ns) for (int k : ks) for (int E : Es) for (int G : Gs) for (int m : ms) {
    const int got = rsx_topk_rows_rules_supported(n, k, E, G, m);
    if (got != expect_supported(n, k, E, G, m)) {
      std::printf("FAILED supported(%d, %d, %d, %d, %d) = %d\n", n, k, E, G, m, got);
      ++fails;
    }
    ++checked;
  }
  EXPECT(rsx_topk_rows_rules_supported(4096, 100, 256, 802, 16) == 1);
  EXPECT(rsx_topk_rows_rules_supported(16384 - 1024, 1024, 0, 802, 1) == 0);
  EXPECT(rsx_topk_rows_rules_supported(13254 - 1024, 1024, 256, 802, 16) == 1);
  EXPECT(rsx_topk_rows_rules_supported(13255 - 1024, 1024, 256, 802, 16) == 0);

  // the refusals: pointers that are never dereferenced on the host (one past small arrays would do; these are plain objects)
  static float scores[32], val[16];
  static int32_t cand[16], excl[8], cate[16], idx[16], state[4];
  static uint32_t allow[2];
  auto call = [&](const float* s, int ld, const int32_t* c, const int32_t* e, int E, const int32_t* g, int G, const uint32_t* a, int m,
                  int U, int n, int k, float* v, int32_t* i, int32_t* st) {
    return rsx_topk_rows_rules(s, ld, c, e, E, g, G, a, m, U, n, k, v, i, st, nullptr);
  };
  EXPECT(call(nullptr, 16, cand, excl, 4, cate, 3, allow, 2, 2, 16, 8, val, idx, state) == RSX_EINVAL);
  EXPECT(call(scores, 16, nullptr, excl, 4, cate, 3, allow, 2, 2, 16, 8, val, idx, state) == RSX_EINVAL);
  EXPECT(call(scores, 16, cand, nullptr, 4, cate, 3, allow, 2, 2, 16, 8, val, idx, state) == RSX_EINVAL);
  EXPECT(call(scores, 16, cand, excl, 4, nullptr, 3, allow, 2, 2, 16, 8, val, idx, state) == RSX_EINVAL);
  EXPECT(call(scores, 16, cand, excl, 4, nullptr, 3, allow, 0, 2, 16, 8, val, idx, state) == RSX_EINVAL);
  EXPECT(call(scores, 16, cand, excl, 4, nullptr, 3, nullptr, 1, 2, 16, 8, val, idx, state) == RSX_EINVAL);
  EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, 2, 2, 16, 8, nullptr, idx, state) == RSX_EINVAL);
  EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, 2, 2, 16, 8, val, nullptr, state) == RSX_EINVAL);
  EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, 2, 2, 16, 8, val, idx, nullptr) == RSX_EINVAL);
  for (int G : {0, -1, INT_MIN}) {
    EXPECT(call(scores, 16, cand, excl, 4, cate, G, allow, 0, 2, 16, 8, val, idx, state) == RSX_EINVAL);
    EXPECT(call(scores, 16, cand, excl, 4, cate, G, nullptr, 1, 2, 16, 8, val, idx, state) == RSX_EINVAL);
  }
  for (int bad : {-1, INT_MIN}) {
    EXPECT(call(scores, 16, cand, excl, bad, cate, 3, allow, 2, 2, 16, 8, val, idx, state) == RSX_EINVAL);      // E
    EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, bad, 2, 16, 8, val, idx, state) == RSX_EINVAL);      // m
    EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, 2, bad, 16, 8, val, idx, state) == RSX_EINVAL);      // U
    EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, 2, 2, bad, 8, val, idx, state) == RSX_EINVAL);       // n
    EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, 2, 2, 16, bad, val, idx, state) == RSX_EINVAL);      // k
  }
  EXPECT(call(scores, 15, cand, excl, 4, cate, 3, allow, 2, 2, 16, 8, val, idx, state) == RSX_EINVAL);          // ld < n
  EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, 17, 2, 16, 8, val, idx, state) == RSX_EUNSUPPORTED);
  EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, INT_MAX, 2, 16, 8, val, idx, state) == RSX_EUNSUPPORTED);
  EXPECT(call(scores, 16, cand, excl, 257, cate, 3, allow, 2, 2, 16, 8, val, idx, state) == RSX_EUNSUPPORTED);
  EXPECT(call(scores, 16, cand, excl, 4, cate, 3, allow, 2, 2, 16, 1025, val, idx, state) == RSX_EUNSUPPORTED);
  EXPECT(call(scores, INT_MAX, cand, excl, 4, cate, 3, allow, 2, 2, INT_MAX, 8, val, idx, state) == RSX_EUNSUPPORTED);
  EXPECT(call(scores, 16376, cand, excl, 4, cate, 802, allow, 1, 2, 16376, 8, val, idx, state) == RSX_EUNSUPPORTED);
  EXPECT(call(scores, 16, cand, excl, 4, cate, INT_MAX, allow, 1, 2, 16, 8, val, idx, state) == RSX_EUNSUPPORTED);
  EXPECT(call(scores, 16, cand, excl, 4, cate, 20000, allow, 1, 2, 16, 8, val, idx, state) == RSX_EUNSUPPORTED);
  std::printf("%ld plans checked, %d failures\n", checked, fails);
  return fails ? 1 : 0;
}
