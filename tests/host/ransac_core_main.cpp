// Stand-alone run of mavmap_amd/csrc/ransac_core.h under the host sanitizers - TEST PROGRAM ONLY, not run through Python:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/ransac_core_main.cpp -o ransac_core_main
// Exit status 1 with a line on stderr: a row that is not strictly ascending or not within range, or a wrong answer.
#include <cstdio>
#include <vector>

#include "../../mavmap_amd/csrc/e5_math.h"

using namespace mavba;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

template <int K>
static void rows(unsigned n) {
  for (unsigned t = 0; t < 4000; ++t) {
    int a[K], s[5] = {0, 0, 0, 0, 0};
    ransac_draw_row<K>(0x1234u + n, t, n, a);
    if constexpr (K == 4) { p3p_sort4(a[0], a[1], a[2], a[3]); p3p_draw_sample(0x1234u + n, t, n, s[0], s[1], s[2], s[3]); }
    else { e5_sort5(a[0], a[1], a[2], a[3], a[4]); e5_draw_sample(0x1234u + n, t, n, s[0], s[1], s[2], s[3], s[4]); }
    for (int k = 0; k < K; ++k) EXPECT(a[k] >= 0 && a[k] < (int)n && (k == 0 || a[k - 1] < a[k]) && a[k] == s[k]);
  }
}

int main() {
  for (unsigned n : {4u, 5u, 6u, 64u}) { rows<4>(n); if (n >= 5) rows<5>(n); }
  const int32_t good[8] = {0, 1, 2, 3, 5, 4, 3, 0}, twice[8] = {0, 1, 2, 3, 5, 4, 5, 0}, out[8] = {0, 1, 2, 3, 6, 4, 3, 0}, neg[4] = {0, -1, 2, 3};
  EXPECT(ransac_check_rows<4>(good, 2, 6) && ransac_check_rows<4>(good, 0, 6) && ransac_check_rows<5>(good, 1, 6));
  EXPECT(!ransac_check_rows<4>(twice, 2, 6) && ransac_check_rows<4>(twice, 1, 6) && !ransac_check_rows<4>(out, 2, 6) && ransac_check_rows<4>(out, 2, 7));
  EXPECT(!ransac_check_rows<4>(neg, 1, 6) && !ransac_check_rows<5>(good, 1, 3));
  for (long long n : {4, 5, 6, 64})
    for (double p : {0.0, 0.99, 1.0})
      for (int size = 4; size <= 5; ++size) {
        int before = kRansacNoLimit;
        for (long long k = 0; k <= n; ++k) {  // more inliers never ask for more trials, a larger sample never for fewer
          const int limit = ransac_dynamic_limit(k, n, size, p);
          EXPECT(limit >= 0 && limit <= before && (size == 4 || limit >= ransac_dynamic_limit(k, n, 4, p)));
          before = limit;
        }
        EXPECT(ransac_dynamic_limit(0, n, size, p) == kRansacNoLimit && ransac_dynamic_limit(n, n, size, p) <= 1);
      }
  // a replay over the table of limits by count: trial 1 leads, trial 2 ties it with the smaller sum, trial 3 is invalid
  // (no inliers), trial 4 ties with a larger sum and ends the run (4 >= table[5]); trial 5 would have won
  const int cnt[6] = {3, 5, 5, 0, 5, 9}, table[10] = {99, 99, 99, 99, 99, 4, 4, 4, 4, 0};
  const double sum[6] = {1.0, 2.0, 1.5, 0.0, 1.7, 0.1};
  RansacSelect sel;
  int t = 0;
  while (t < 6 && !ransac_select_step(sel, t, t & 1, t != 3, cnt[t], sum[t], table[cnt[t]], 0)) ++t;
  EXPECT(t == 4 && sel.best_trial == 2 && sel.best_model == 0 && sel.best_inliers == 5 && sel.best_sum == 1.5 && sel.trials_used == 5);
  RansacSelect stop;
  EXPECT(!ransac_select_step(stop, 0, 0, true, 3, 1.0, 99, 4) && ransac_select_step(stop, 1, 0, true, 4, 1.0, 99, 4) && stop.best_trial == 1);
  std::printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
