/* od_buf.cuh - the owners of the library's host-side GPU buffers.

   DeviceBuf<T> (hipMalloc) and PinnedBuf<T> (hipHostMalloc, hipHostMallocDefault) hold one
   buffer of `cap` elements each: freed by the destructor, never copied, movable (so that an
   element of a std::vector may own some).  The capacity only grows and is exactly what was last
   asked for; a failed allocation leaves p == nullptr and cap == 0.

   Everything is in an anonymous namespace, as in od_band_stage.cuh, which includes this. */
#pragma once
#include "od_common.cuh"

namespace {

/* Owners of device resources are never copied. */
struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy &) = delete;
  NoCopy &operator=(const NoCopy &) = delete;
};

template <class T, bool Pinned>
struct GpuBuf : NoCopy {
  T *p = nullptr;
  size_t cap = 0;   /* elements */
  GpuBuf() = default;
  GpuBuf(GpuBuf &&o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  GpuBuf &operator=(GpuBuf &&o) noexcept {
    if (this != &o) {
      if (p) (void)release(p);
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~GpuBuf() {
    if (p) (void)release(p);
  }
  static hipError_t release(T *q) { return Pinned ? hipHostFree(q) : hipFree(q); }
  /* frees the buffer now (hipFree waits for the device) */
  int drop() {
    if (p) ODHIP_TRY(release(p));
    p = nullptr;
    cap = 0;
    return ODHIP_SUCCESS;
  }
  int alloc(size_t n) {
    const hipError_t e = Pinned ? hipHostMalloc((void **)&p, n*sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, n*sizeof(T));
    if (e != hipSuccess) p = nullptr;
    ODHIP_TRY(e);
    cap = n;
    return ODHIP_SUCCESS;
  }
  /* at least n elements, for a caller whose stream has drained: the old buffer is freed first */
  int reserve(size_t n) {
    if (n <= cap) return ODHIP_SUCCESS;
    const int rc = drop();
    return rc ? rc : alloc(n);
  }
  /* at least n elements; the old buffer is freed once nothing queued on the caller's stream can still use it */
  int grow(size_t n, hipStream_t s) {
    if (n <= cap) return ODHIP_SUCCESS;
    ODHIP_TRY(hipStreamSynchronize(s));
    return reserve(n);
  }
};

template <class T>
using DeviceBuf = GpuBuf<T, false>;
template <class T>
using PinnedBuf = GpuBuf<T, true>;

}  // namespace
