// ransac_core.h — what the RANSAC calls share whatever their hypothesis is: the sample generator, the dynamic trial
// limit, the selection among the trials and the per-item record of the kernels. p3p_math.h (rows of four) and
// e5_math.h (rows of five) include it; like them it is __host__ __device__ and compiles under g++. What really differs
// stays with the callers: which items run (n > 4 / n > 5), the least consensus (4 / 5 inliers), what trials_used
// reports when no trial ended the run, the threshold, and what an invalid trial counts as.
//
// What is evaluated (reference file:line):
//   samples       src/util/estimation.cc:71-93: distinct indices, used in ascending order (std::set); the generator
//                 itself is this library's (include/mavba_absolute_pose.h writes its recipe out)
//   selection     src/util/estimation.cc:15-21, :119-133
#ifndef MAVBA_RANSAC_CORE_H_
#define MAVBA_RANSAC_CORE_H_

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "ba_math.h"

namespace mavba {

constexpr int kRansacNoLimit = 0x7fffffff;  // entry of the dynamic-limit table: no limit
constexpr int kRansacMaxDraws = 64;         // draws of the generator before a row is completed in order

// ---------------------------------------------------------------------------
// Samples
// ---------------------------------------------------------------------------
MAVBA_HD unsigned long long ransac_mix(unsigned long long seed, unsigned trial, unsigned draw) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (((unsigned long long)trial << 32) + (unsigned long long)draw + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

MAVBA_HD void cswap(int& a, int& b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo; b = hi;
}

// appends v to the row (a[0..K), cnt entries) unless the row holds it (fully unrolled, selects and not branches: the
// row stays in registers)
template <int K>
MAVBA_HD void ransac_row_add(int v, int* a, int& cnt) {
  bool add = true;
#pragma unroll
  for (int k = 0; k < K; ++k) add = add && v != a[k];
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = add && cnt == k ? v : a[k];
  cnt += add ? 1 : 0;
}

// The K distinct indices of trial `trial` for n >= K points, in the order drawn: the caller sorts them with its network.
template <int K>
MAVBA_HD void ransac_draw_row(unsigned long long seed, unsigned trial, unsigned n, int* a) {
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = -1;
  int cnt = 0;
  for (unsigned d = 0; d < (unsigned)kRansacMaxDraws && cnt < K; ++d)
    ransac_row_add<K>((int)(((ransac_mix(seed, trial, d) >> 32) * (unsigned long long)n) >> 32), a, cnt);
  for (int v = 0; cnt < K; ++v) ransac_row_add<K>(v, a, cnt);
}

// Supplied rows [max_trials][K] of an item with n points: false if one holds an index twice or one outside [0, n). (HOST)
template <int K>
inline bool ransac_check_rows(const int32_t* samples, int max_trials, long long n) {
  for (long long r = 0; r < (long long)K * max_trials; r += K) {
    const int32_t* s = samples + r;
    bool bad = false;
    for (int a = 0; a < K; ++a) {
      bad |= s[a] < 0 || s[a] >= n;
      for (int b = 0; b < a; ++b) bad |= s[a] == s[b];
    }
    if (bad) return false;
  }
  return true;
}

// ---------------------------------------------------------------------------
// Selection
// ---------------------------------------------------------------------------
struct RansacSelect {
  long long best_inliers = 0;
  double best_sum = DBL_MAX;
  int best_trial = -1, best_model = -1;
  int trials_used = 0;
};

// estimation.cc:119-133 for model m of trial t (one model per trial: m = 0). `limit` = the dynamic-limit table at THIS
// model's count. Returns true when the run ends with this model (the later models of the trial are then ignored).
// A model that is not `valid` never becomes the best and counts as one with no inliers.
MAVBA_HD bool ransac_select_step(RansacSelect& s, int t, int m, bool valid, int num_inliers, double residual_sum, int limit,
                                 long long stop_num_inliers) {
  if (valid && (num_inliers > s.best_inliers || (num_inliers == s.best_inliers && residual_sum < s.best_sum))) {
    s.best_inliers = num_inliers;
    s.best_sum = residual_sum;
    s.best_trial = t;
    s.best_model = m;
  }
  s.trials_used = t + 1;
  return (stop_num_inliers > 0 && s.best_inliers >= stop_num_inliers) || t >= limit;
}

// dynamic_max_trials_(k, n, sample_size, probability) as a table entry, with the HOST's log / pow / ceil (a device pow
// that differs by one ulp would flip a ceil): a quotient that is not finite means no limit, a finite one is clamped.
inline int ransac_dynamic_limit(long long k, long long n, int sample_size, double probability) {
  const double e = 1 - k / (double)n;
  const double nom = fmax(DBL_MIN, 1 - probability);
  const double denom = fmax(DBL_MIN, 1 - pow(1 - e, (double)sample_size));
  const double quot = ceil(log(nom) / log(denom));
  if (!(quot - quot == 0.0)) return kRansacNoLimit;
  return quot <= 0.0 ? 0 : (quot >= (double)kRansacNoLimit ? kRansacNoLimit : (int)quot);
}

// One item of a batch as the kernels read it (uniform: scalar loads). As initialised here the item does not run:
// it owns no work-group and the host answers it.
struct RansacItemDev {
  long long pt_begin = 0;        // first point of the item in the packed arrays
  long long trial_begin = 0;     // first trial of the item in the per-trial arrays
  long long table_begin = 0;     // first entry (k = 0) of the item's dynamic-limit table
  long long samples_begin = -1;  // first row of the item's supplied samples, or -1: draw them
  long long stop = 0;            // stop_num_inliers, <= 0: none
  unsigned long long seed = 0;
  double thr = 0.0;              // the threshold in normalised coordinates
  int n = 0, max_trials = 0, first_block = 0, num_blocks = 0;
};

}  // namespace mavba
#endif  // MAVBA_RANSAC_CORE_H_
