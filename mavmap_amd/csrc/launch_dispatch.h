// launch_dispatch.h - a run-time value as a compile-time constant, for the launch wrappers that pick a kernel instantiation.
//   with_width(kmax, [&](auto k) { constexpr int K = decltype(k)::value; ... k_some_kernel<K> ... });
// Every f is instantiated for ALL values of its helper; a combination that must not exist is left out with `if constexpr`.
#ifndef MAVBA_LAUNCH_DISPATCH_H_
#define MAVBA_LAUNCH_DISPATCH_H_
#include <type_traits>

namespace mavba {

// The width class of the widest camera model among the free intrinsics: 4 (PINHOLE), 8 (OPENCV) or 9 parameters.
template <class F>
inline void with_width(int kmax, F&& f) {
  if (kmax <= 4) f(std::integral_constant<int, 4>{});
  else if (kmax <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 9>{});
}
// The same with class 0 in front: no intrinsics block is free.
template <class F>
inline void with_width_or_none(int kmax, F&& f) {
  if (kmax <= 0) f(std::integral_constant<int, 0>{});
  else with_width(kmax, f);
}
template <class F>
inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace mavba
#endif
