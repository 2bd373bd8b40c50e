// dev_buf.hpp -- a device allocation that its holder owns (the scene's arrays and per-render scratch behind the C ABI, the scratch of the
// device tree builder).  Nothing but the HIP runtime: bvh_gpu.hip includes it without the ABI headers.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace pbrt_hip {
// A device allocation that the buffer owns: freed by its destructor, on whichever device is current then.  n and p change only
// when hipMalloc succeeds; after a failure the buffer is empty (n == 0, p == nullptr), so a later grow() tries again.
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf &operator=(DevBuf o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }  // (moves only: o is moved into)
  ~DevBuf() { release(); }
  // frees what the buffer holds and allocates `count` elements (contents undefined)
  hipError_t alloc(size_t count) {
    release();
    if (count == 0) return hipSuccess;
    T *q = nullptr;
    const hipError_t e = hipMalloc((void **)&q, count * sizeof(T));
    if (e == hipSuccess) { p = q; n = count; }
    return e;
  }
  // grow-only scratch: allocated anew (contents lost) when it holds fewer than `need` elements
  hipError_t grow(size_t need) { return n < need ? alloc(need) : hipSuccess; }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};
}  // namespace pbrt_hip
