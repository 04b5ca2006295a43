// Host build (g++) of mavmap_amd/csrc/h4_math.h — TEST HARNESS ONLY.
// Lets the CPU test-suite check the bodies of the homography kernel without a GPU, and gives the one-thread host
// time the timing script compares the kernel with.
#include "../../include/mavba_homography.h"
#include "../../mavmap_amd/csrc/h4_math.h"

extern "C" {
void hh_draw_samples(unsigned long long seed, long long n, int trials, int* out) {
  for (int t = 0; t < trials; ++t) mavba::h4_draw_sample(seed, (unsigned)t, (unsigned)n, out + 4 * t);
}
// count hypotheses: m [count][4][4] matches (x, y, u, v) in sample order, H [count][9], valid [count]
void hh_estimate(long long count, const double* m, double* H, unsigned char* valid) {
  for (long long i = 0; i < count; ++i) valid[i] = mavba::h4_estimate(reinterpret_cast<const double (*)[4]>(m + 16 * i), H + 9 * i) ? 1 : 0;
}
int hh_dynamic_limit(long long k, long long n, double probability) { return mavba::h4_dynamic_limit(k, n, probability); }
// One item as the kernel runs it, on one thread.
void hh_homography(mavba_homography_item* it) { mavba::h4_run_item(*it); }
}
