// batch_call.h - the host frame of a stand-alone batched call (triangulate.hip, absolute_pose.hip, relative_pose.hip,
// pose_refine.hip and the stand-alone entries of api.hip and scene.hip). HIP host code: not part of the g++ harnesses.
// Such a call reads as five steps - validate its own fields, pack its own arrays, launch, download, scatter - and keeps:
//   1. Arguments are judged before the device is touched: an invalid call says so on any machine, also one without a GPU.
//   2. No memory of the caller's is written before the last download has succeeded: an error leaves every output untouched.
//   3. The caller's current device is restored on return, on every path.
#ifndef MAVBA_BATCH_CALL_H_
#define MAVBA_BATCH_CALL_H_
#include <new>

#include "session.h"
#include "ransac_core.h"

namespace mavba {

// ---- the shared argument checks (rule 1) and their messages ----
constexpr long long kBatchMax = 0x7fffffffLL;  // what one batch may hold of anything the kernels index with an int

// n in [0, 2^31) and `rest`: what else the call requires of the item (its pointers when n > 0, max_trials >= 0)
inline void check_item(long long n, bool rest, const char* what) {
  if (n < 0 || n > kBatchMax || !rest) throw Failure(MAVBA_ERR_INVALID_ARGUMENT, std::string("null or negative argument in ") + what + " item");
}
inline void check_model(int model) { if (model < 1 || model > 3) throw Failure(MAVBA_ERR_BAD_MODEL, "bad camera model"); }
inline void require_device() { if (mavba_device_count() <= 0) throw Failure(MAVBA_ERR_NO_DEVICE, "no HIP device: the mavba backend has no CPU path"); }

// The running totals of a RANSAC batch while its items are judged in order.
struct RansacBatch {
  long long points = 0, trials = 0, blocks = 0, table_len = 0, rows = 0;
  // Places an item that runs (which ones do is the call's own rule) behind the ones before it and checks its supplied
  // rows. K: the sample size; model_doubles: what one trial takes in the array of models.
  template <int K>
  void place(RansacItemDev& d, long long n, int max_trials, long long stop, unsigned long long seed, const int32_t* samples,
             int trials_per_group, int model_doubles) {
    d.pt_begin = points; d.trial_begin = trials; d.table_begin = table_len; d.stop = stop; d.seed = seed;
    d.n = (int)n; d.max_trials = max_trials; d.first_block = (int)blocks;
    d.num_blocks = (max_trials + trials_per_group - 1) / trials_per_group;
    if (samples) {
      if (!ransac_check_rows<K>(samples, max_trials, n)) throw Failure(MAVBA_ERR_INVALID_ARGUMENT, "sample row with a repeated or out-of-range index");
      d.samples_begin = rows;
      rows += max_trials;
    }
    points += n; trials += max_trials; blocks += d.num_blocks; table_len += n + 1;
    if (points > kBatchMax || trials > kBatchMax / model_doubles || blocks > kBatchMax || table_len > kBatchMax)
      throw Failure(MAVBA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 points, model entries or work-groups in one batch");
  }
};

// block_map[g] = (item, work-group of the item) from the items' (first_block, num_blocks); an item may own none
template <typename Item>
std::vector<int2> make_block_map(const std::vector<Item>& items, long long blocks) {
  std::vector<int2> map((size_t)blocks);
  for (size_t q = 0; q < items.size(); ++q)
    for (int c = 0; c < items[q].num_blocks; ++c) map[(size_t)items[q].first_block + c] = make_int2((int)q, c);
  return map;
}

// ---- scopes (rule 3) ----
// Runs on `device` if that is >= 0 and gives the calling thread its device back on exit. A thread whose current device
// cannot be read gets nothing back.
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int device) {
    if (device < 0) return;
    const int cur = current();
    if (cur != device) { HIP_OK(hipSetDevice(device)); prev = cur; }
  }
  // for a tear-down, which goes on where it is when the device cannot be selected
  DeviceScope(int device, const std::nothrow_t&) noexcept {
    const int cur = current();
    if (cur >= 0 && cur != device && hipSetDevice(device) == hipSuccess) prev = cur;
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  static int current() {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = -1; }
    return cur;
  }
};

// The cached stream of the current device for the length of one call. On exit, on every path: the events destroyed,
// the stream synchronised, its staging blocks returned, the stream back in the cache.
struct StreamScope {
  hipStream_t st = nullptr;
  int dev = 0;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  StreamScope() { HIP_OK(hipGetDevice(&dev)); HIP_OK(stream_acquire(&st)); }
  ~StreamScope() {
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
    (void)hipStreamSynchronize(st); release_staged(st); stream_release(st, dev);
  }
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
  // around the launch (optional): the pair of events seconds() reads, and the launch's own error
  void begin() { HIP_OK(hipEventCreate(&ev_a)); HIP_OK(hipEventCreate(&ev_b)); HIP_OK(hipEventRecord(ev_a, st)); }
  void end() { HIP_OK(hipGetLastError()); HIP_OK(hipEventRecord(ev_b, st)); }
  // "resize and copy if some item asked for it": count elements of T from src, returns with the data in h
  template <typename T>
  void download(std::vector<T>& h, const void* src, size_t count, bool wanted = true) {
    if (!wanted) return;
    h.resize(count);
    HIP_OK(copy_d2h_staged_sync(h.data(), src, count * sizeof(T), st));
  }
  // behind the last download (which synchronised): the staging blocks go back and an error of the stream's work is
  // reported BEFORE the caller's memory is written (rule 2)
  void finish() { release_staged(st); HIP_OK(hipGetLastError()); }
  double seconds() {  // of the launch between begin() and end(); behind finish()
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, ev_a, ev_b));
    return 1e-3 * (double)ms;
  }
};

}  // namespace mavba
#endif  // MAVBA_BATCH_CALL_H_
