// Stand-alone run of mavmap_amd/csrc/match_math.h under the host sanitizers - TEST PROGRAM ONLY, not run through Python:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/match_math_main.cpp -o match_math_main
// The small sizes of the grid of tests/test_match_host.py, with and without the spatial mask, and the items the host
// answers, through the one-thread item run. Exit status 1 with a line on stderr: a guard behind an output overwritten,
// an index out of range, neighbours or matches out of order, a match the cross-check does not allow.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/mavba_match.h"
#include "../../mavmap_amd/csrc/match_math.h"

using namespace mavba;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static unsigned long long state = 2024;
static double unit() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.0; }

static void run(long long n1, long long n2, int dim, double max_ratio, double max_distance, bool with_xy) {
  const size_t cap = (size_t)(n1 < n2 ? n1 : n2);
  std::vector<float> d1((size_t)n1 * dim + 1), d2((size_t)n2 * dim + 1), xy1(2 * (size_t)n1 + 1), xy2(2 * (size_t)n2 + 1);
  for (float& v : d1) v = (float)(unit() - 0.5);
  for (float& v : d2) v = (float)(unit() - 0.5);
  for (long long j = 0; j < n2 && j < n1; j += 2)  // every second keypoint of image 2 is a noisy copy of one of image 1
    for (int k = 0; k < dim; ++k) d2[(size_t)j * dim + k] = d1[(size_t)((j * 7) % n1) * dim + k] + (float)(0.02 * (unit() - 0.5));
  for (float& v : xy1) v = (float)(100.0 * unit());
  for (float& v : xy2) v = (float)(100.0 * unit());
  std::vector<int32_t> matches(2 * cap + 1, -7), nn12(2 * (size_t)n1 + 1, -7), nn21(2 * (size_t)n2 + 1, -7);
  std::vector<float> distances(cap + 1, -7.0f), dist12(2 * (size_t)n1 + 1, -7.0f), dist21(2 * (size_t)n2 + 1, -7.0f);
  mavba_match_item it = mavba_match_item();
  it.desc1 = d1.data(); it.desc2 = d2.data(); it.xy1 = with_xy ? xy1.data() : nullptr; it.xy2 = with_xy ? xy2.data() : nullptr;
  it.n1 = n1; it.n2 = n2; it.dim = dim; it.max_ratio = max_ratio; it.max_distance = max_distance;
  it.matches = matches.data(); it.distances = distances.data(); it.nn12 = nn12.data(); it.dist12 = dist12.data();
  it.nn21 = nn21.data(); it.dist21 = dist21.data();
  it.num_matches = -7;
  match_run_item(it);
  EXPECT(matches[2 * cap] == -7 && nn12[2 * (size_t)n1] == -7 && nn21[2 * (size_t)n2] == -7);
  EXPECT(distances[cap] == -7.0f && dist12[2 * (size_t)n1] == -7.0f && dist21[2 * (size_t)n2] == -7.0f);
  EXPECT(it.num_matches >= 0 && (size_t)it.num_matches <= cap);
  if (n1 < 2 || n2 < 2) {
    EXPECT(it.num_matches == 0 && std::isnan(it.median_disparity));
    for (long long i = 0; i < 2 * n1; ++i) EXPECT(nn12[(size_t)i] == -1 && std::isnan(dist12[(size_t)i]));
    for (long long j = 0; j < 2 * n2; ++j) EXPECT(nn21[(size_t)j] == -1 && std::isnan(dist21[(size_t)j]));
    return;
  }
  auto side = [&](const std::vector<int32_t>& nn, const std::vector<float>& dist, long long n, long long other) {
    for (long long i = 0; i < n; ++i) {
      const int a = nn[2 * (size_t)i], b = nn[2 * (size_t)i + 1];
      EXPECT(a >= -1 && a < other && b >= -1 && b < other && (a >= 0 || b < 0) && (a < 0 || a != b));
      EXPECT((a < 0) == std::isnan(dist[2 * (size_t)i]) && (b < 0) == std::isnan(dist[2 * (size_t)i + 1]));
      if (b >= 0) EXPECT(dist[2 * (size_t)i] < dist[2 * (size_t)i + 1] || (dist[2 * (size_t)i] == dist[2 * (size_t)i + 1] && a < b));
      if (max_distance < 0) EXPECT(b >= 0);
    }
  };
  side(nn12, dist12, n1, n2);
  side(nn21, dist21, n2, n1);
  for (int q = 0; q < it.num_matches; ++q) {
    const int i = matches[2 * (size_t)q], j = matches[2 * (size_t)q + 1];
    EXPECT(i >= 0 && i < n1 && j >= 0 && j < n2 && (q == 0 || matches[2 * (size_t)q - 2] < i));
    EXPECT(nn12[2 * (size_t)i] == j && nn21[2 * (size_t)j] == i && nn12[2 * (size_t)i + 1] >= 0 && nn21[2 * (size_t)j + 1] >= 0);
    EXPECT(distances[(size_t)q] == dist12[2 * (size_t)i] && distances[(size_t)q] == dist21[2 * (size_t)j]);  // d2(i, j) and d2(j, i): the same bits
    EXPECT(!((double)(dist12[2 * (size_t)i] / dist12[2 * (size_t)i + 1]) > max_ratio));
  }
  EXPECT(std::isnan(it.median_disparity) == (it.num_matches == 0 || !with_xy));
  if (max_ratio >= 1.0 && max_distance < 0) EXPECT(it.num_matches > 0);
}

int main() {
  const long long sizes[] = {2, 3, 15, 16, 17, 63, 64, 65};
  const int dims[] = {4, 60, 64, 128};
  int c = 0;
  for (long long n1 : sizes)
    for (long long n2 : sizes) {
      const int dim = dims[c++ % 4];
      run(n1, n2, dim, 0.9, -1.0, c % 3 != 0);
      run(n1, n2, dim, 0.9, 40.0, true);
    }
  run(65, 17, 128, 1.0, -1.0, true);
  run(17, 65, 64, 0.0, -1.0, true);
  run(64, 64, 64, 0.9, 0.0, true);  // every pair masked
  run(0, 0, 64, 0.9, -1.0, false);
  run(1, 64, 64, 0.9, -1.0, true);
  run(64, 1, 128, 0.9, 40.0, true);
  run(0, 5, 4, 0.9, -1.0, false);
  std::printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
