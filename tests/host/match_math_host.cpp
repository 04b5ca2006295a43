// Host build (g++) of mavmap_amd/csrc/match_math.h — TEST HARNESS ONLY.
// Lets the CPU test-suite check the bodies of the matching kernels without a GPU, and gives the one-thread host
// time the timing script compares the kernels with.
#include "../../include/mavba_match.h"
#include "../../mavmap_amd/csrc/match_math.h"

extern "C" {
// d2 [n1][n2] by rule 2
void mh_d2(const float* a, long long n1, const float* b, long long n2, int dim, float* out) {
  for (long long i = 0; i < n1; ++i)
    for (long long j = 0; j < n2; ++j) out[i * n2 + j] = mavba::match_d2(a + i * dim, b + j * dim, dim);
}
// mask [n1][n2] by rule 1 (max_distance >= 0)
void mh_mask(const float* xy1, long long n1, const float* xy2, long long n2, double max_distance, unsigned char* out) {
  const double md2 = max_distance * max_distance;
  for (long long i = 0; i < n1; ++i)
    for (long long j = 0; j < n2; ++j) out[i * n2 + j] = mavba::match_candidate(xy1[2 * i], xy1[2 * i + 1], xy2[2 * j], xy2[2 * j + 1], md2) ? 1 : 0;
}
// One item by rules 1-6, exhaustively, on one thread.
void mh_match(mavba_match_item* it) { mavba::match_run_item(*it); }
}
