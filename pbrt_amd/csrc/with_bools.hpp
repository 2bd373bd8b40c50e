// with_bools.hpp -- the kernel units' launchers turn run-time switches into template arguments:
// with_bools(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...)
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace pbrt_hip {
template <class F>
static hipError_t with_bools(F &&f) { return f(); }
template <class F, class... Bs>
static hipError_t with_bools(F &&f, bool b, Bs... rest) {
  if (b) return with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
  return with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}
}  // namespace pbrt_hip
