// Host build (g++) of mavmap_amd/csrc/tri_math.h — TEST HARNESS ONLY.
// Lets the CPU test-suite check the bodies of the triangulation kernel without a GPU.
#include "../../mavmap_amd/csrc/tri_math.h"
extern "C" {
void ht_image2world(int model, const double* cam, long long n, const double* uv, double* xy) {
  for (long long i = 0; i < n; ++i) mavba::image2world(model, cam, uv[2 * i], uv[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
}
double ht_threshold(double threshold, const double* cam) { return mavba::image2world_threshold(threshold, cam); }
void ht_world2image(int model, const double* cam, const double* Xc, double* uv) {
  mavba::project<false>(model, cam, Xc, uv[0], uv[1], nullptr, nullptr);
}
void ht_pair_prepare(const double* rvec1, const double* tvec1, const double* rvec2, const double* tvec2, double* rec) {
  mavba::tri_pair_prepare(rvec1, tvec1, rvec2, tvec2, rec);
}
// xy1 / xy2: normalised points. h [n][4] unit homogeneous vectors, X [n][3], sweeps [n].
void ht_dlt(const double* rec, long long n, const double* xy1, const double* xy2, double* h, double* X, int* sweeps) {
  for (long long i = 0; i < n; ++i)
    sweeps[i] = mavba::triangulate_dlt(rec, rec + 12, xy1[2 * i], xy1[2 * i + 1], xy2[2 * i], xy2[2 * i + 1], h + 4 * i, X + 3 * i);
}
// The whole per-correspondence path of one pair, as the kernel runs it (one thread = one i). out [n][7] =
// { X[3], angle, err, depth1, depth2 }. Returns the number accepted.
long long ht_pair(const double* rvec1, const double* tvec1, const double* rvec2, const double* tvec2, int model1, const double* cam1,
                  int model2, const double* cam2, long long n, const double* uv1, const double* uv2, const unsigned char* has_xyz,
                  const double* xyz_in, double max_reproj_error_px, double min_angle_deg, int reject_bits, double* out, int* status,
                  unsigned char* accept) {
  double rec[mavba::kTriRec];
  mavba::tri_pair_prepare(rvec1, tvec1, rvec2, tvec2, rec);
  const double thr_n = mavba::image2world_threshold(max_reproj_error_px, cam2);
  const double min_angle_rad = mavba::tri_min_angle_rad(min_angle_deg);
  long long count = 0;
  for (long long i = 0; i < n; ++i) {
    bool acc;
    const bool have = has_xyz && has_xyz[i];
    status[i] = mavba::tri_correspondence(rec, model1, cam1, model2, cam2, uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1], have,
                                          have ? xyz_in + 3 * i : nullptr, thr_n, min_angle_rad, reject_bits, out + 7 * i, acc);
    accept[i] = acc ? 1 : 0;
    count += acc;
  }
  return count;
}
}
