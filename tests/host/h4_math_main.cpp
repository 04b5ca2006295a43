// Stand-alone run of mavmap_amd/csrc/h4_math.h under the host sanitizers - TEST PROGRAM ONLY, not run through Python:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/h4_math_main.cpp -o h4_math_main
// Every degenerate input of tests/test_homography_host.py and one case of its grid through the one-thread item run.
// Exit status 1 with a line on stderr: a NaN model marked valid, an invalid trial with a count or a sum, a wrong answer.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/mavba_homography.h"
#include "../../mavmap_amd/csrc/h4_math.h"

using namespace mavba;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Run {
  std::vector<double> uv1, uv2, models, sums;
  std::vector<int32_t> samples, counts, rows;
  std::vector<uint8_t> mask;
  mavba_homography_item it;
};

// uv1 / uv2: n matches; rows: supplied samples (empty: drawn)
static Run run(std::vector<double> uv1, std::vector<double> uv2, int max_trials, long long stop, std::vector<int32_t> samples = {}) {
  Run r;
  r.uv1 = std::move(uv1); r.uv2 = std::move(uv2); r.samples = std::move(samples);
  const size_t n = r.uv1.size() / 2, mt = (size_t)(max_trials > 0 ? max_trials : 0);
  r.models.assign(9 * mt + 1, -7.0); r.sums.assign(mt + 1, -7.0); r.counts.assign(mt + 1, -7); r.rows.assign(4 * mt + 1, -7); r.mask.assign(n + 1, 9);
  mavba_homography_item& it = r.it;
  it = mavba_homography_item();
  it.uv1 = r.uv1.data(); it.uv2 = r.uv2.data(); it.n = (int64_t)n; it.max_reproj_error_px = 4.0; it.max_trials = max_trials;
  it.stop_num_inliers = stop; it.probability = 0.99; it.samples = r.samples.empty() ? nullptr : r.samples.data(); it.seed = 5;
  it.inlier_mask = r.mask.data(); it.trial_models = r.models.data(); it.trial_num_inliers = r.counts.data();
  it.trial_residual_sum = r.sums.data(); it.trial_samples = r.rows.data();
  h4_run_item(it);
  // what holds for every input: the guards behind the arrays are untouched, invalid = all NaN with count 0 and sum 0
  EXPECT(r.models[9 * mt] == -7.0 && r.sums[mt] == -7.0 && r.counts[mt] == -7 && r.rows[4 * mt] == -7 && r.mask[n] == 9);
  for (size_t t = 0; t < mt; ++t) {
    int nans = 0;
    for (int k = 0; k < 9; ++k) nans += std::isnan(r.models[9 * t + k]) ? 1 : 0;
    bool finite = true;
    for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(r.models[9 * t + k]);
    EXPECT(nans == 0 || nans == 9);
    EXPECT(finite || nans == 9);
    if (nans == 9) EXPECT(r.counts[t] == 0 && r.sums[t] == 0.0);
    else EXPECT(r.models[9 * t + 8] == 1.0 && r.counts[t] >= 0 && r.counts[t] <= (int)n && r.sums[t] >= 0.0);
  }
  if (it.status == MAVBA_HOMOGRAPHY_OK) {
    EXPECT(it.best_trial >= 0 && it.best_trial < it.trials_used && it.trials_used <= max_trials && it.num_inliers >= 4);
    EXPECT(it.num_inliers == r.counts[(size_t)it.best_trial] && it.inlier_ratio == it.num_inliers / (double)n);
    int in_mask = 0;
    for (size_t i = 0; i < n; ++i) in_mask += r.mask[i];
    EXPECT(in_mask == it.num_inliers);
    for (int k = 0; k < 9; ++k) EXPECT(it.H[k] == r.models[9 * (size_t)it.best_trial + k]);
  } else {
    EXPECT(it.status == MAVBA_HOMOGRAPHY_NO_CONSENSUS && it.best_trial == -1 && it.num_inliers == 0 && it.inlier_ratio == 0.0 && std::isnan(it.H[0]) && std::isnan(it.H[8]));
    for (size_t i = 0; i < n; ++i) EXPECT(r.mask[i] == 0);
  }
  return r;
}

// n matches of the homography (1.02 x + 0.01 y + 5, -0.02 x + 0.97 y - 8) / (1 + 2e-5 x - 1e-5 y), every seventh an outlier
static void planar(int n, std::vector<double>& uv1, std::vector<double>& uv2) {
  unsigned long long s = 12345;
  auto unit = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
  for (int i = 0; i < n; ++i) {
    const double x = 20 + 712 * unit(), y = 20 + 440 * unit();
    const double w = 1 + 2e-5 * x - 1e-5 * y;
    double u = (1.02 * x + 0.01 * y + 5) / w + (unit() - 0.5), v = (-0.02 * x + 0.97 * y - 8) / w + (unit() - 0.5);
    if (i % 7 == 6) { u += 40; v -= 25; }
    uv1.push_back(x); uv1.push_back(y); uv2.push_back(u); uv2.push_back(v);
  }
}

int main() {
  std::vector<int32_t> rows0123;
  for (int t = 0; t < 8; ++t) for (int k = 0; k < 4; ++k) rows0123.push_back(k);
  std::vector<double> a, b;
  planar(6, a, b);
  {  // all four collinear
    std::vector<double> l1, l2;
    for (int i = 0; i < 6; ++i) { l1.push_back(50 + 130.0 * i); l1.push_back(40 + 78.0 * i); l2.push_back(55 + 128.0 * i); l2.push_back(30 + 80.0 * i); }
    run(l1, l2, 8, 0);
  }
  {  // two identical matches sampled
    std::vector<double> t1 = a, t2 = b;
    t1[2] = t1[0]; t1[3] = t1[1]; t2[2] = t2[0]; t2[3] = t2[1];
    const Run r = run(t1, t2, 8, 0, rows0123);
    for (int t = 1; t < 8; ++t) for (int k = 0; k < 9; ++k) EXPECT(std::isnan(r.models[k]) == std::isnan(r.models[9 * t + k]));  // the same row, the same answer
  }
  {  // all matches identical
    std::vector<double> s1, s2;
    for (int i = 0; i < 6; ++i) { s1.push_back(a[0]); s1.push_back(a[1]); s2.push_back(b[0]); s2.push_back(b[1]); }
    run(s1, s2, 8, 0);
  }
  {  // n = 4, n = 0, max_trials = 0: answered without a run
    Run r = run(std::vector<double>(a.begin(), a.begin() + 8), std::vector<double>(b.begin(), b.begin() + 8), 8, 0);
    EXPECT(r.it.status == MAVBA_HOMOGRAPHY_NO_CONSENSUS && r.it.trials_used == 0 && r.rows[0] == -1 && r.rows[31] == -1 && std::isnan(r.models[0]) && r.counts[7] == 0);
    r = run({}, {}, 8, 0);
    EXPECT(r.it.status == MAVBA_HOMOGRAPHY_NO_CONSENSUS && r.it.trials_used == 0 && r.it.inlier_ratio == 0.0 && r.rows[31] == -1);
    r = run(a, b, 0, 0);
    EXPECT(r.it.status == MAVBA_HOMOGRAPHY_NO_CONSENSUS && r.it.trials_used == 0 && r.mask[5] == 0);
  }
  {  // a NaN coordinate
    std::vector<double> n1 = a;
    n1[4] = NAN;
    const Run r = run(n1, b, 8, 0);
    EXPECT(r.mask[2] == 0);
    for (int t = 0; t < 8; ++t)
      for (int k = 0; k < 4; ++k) if (r.rows[4 * t + k] == 2) EXPECT(std::isnan(r.models[9 * t]));
  }
  {  // the model of matches 0-3 sends match 4 (x = 128) to infinity: its third component is 0
    const double x[6] = {0, 32, 64, 96, 128, 16}, y[6] = {0, 64, 0, 32, 16, 16};
    std::vector<double> f1, f2;
    for (int i = 0; i < 6; ++i) {
      const double w = i == 4 ? 1.0 : 1.0 - x[i] / 128.0;
      f1.push_back(x[i]); f1.push_back(y[i]); f2.push_back(i == 4 ? 0.0 : x[i] / w); f2.push_back(y[i] / w);
    }
    const Run r = run(f1, f2, 8, 0, rows0123);
    EXPECT(r.it.status == MAVBA_HOMOGRAPHY_OK && r.it.num_inliers == 5 && r.mask[4] == 0);
  }
  {  // one case of the grid: 65 matches, 64 trials, drawn rows, a stop at 70 %; and the same with no stop
    std::vector<double> g1, g2;
    planar(65, g1, g2);
    const Run r = run(g1, g2, 64, 45);
    EXPECT(r.it.status == MAVBA_HOMOGRAPHY_OK && r.it.num_inliers >= 45 && r.it.trials_used < 64);
    for (int t = 0; t < 64; ++t) {
      int row[4];
      h4_draw_sample(5, (unsigned)t, 65u, row);
      for (int k = 0; k < 4; ++k) EXPECT(r.rows[4 * t + k] == row[k] && (k == 0 || row[k - 1] < row[k]) && row[k] >= 0 && row[k] < 65);
    }
    const Run q = run(g1, g2, 64, 0);
    EXPECT(q.it.status == MAVBA_HOMOGRAPHY_OK && q.it.num_inliers >= r.it.num_inliers && q.it.trials_used >= r.it.trials_used);
  }
  std::printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
