// fl_devbuf.h -- the one type that owns device memory for the handles that borrow a fl_poisson (fl_ibm, fl_momentum, fl_scalar): a handle whose
// arrays are DevBufs frees them by being deleted, and a new array needs no line in a destroy function.
#pragma once
#include <utility>

#include "fl_handle.h"

#pragma GCC visibility push(hidden)  // internal to the library: its dynamic symbols stay the C-ABI's

namespace fl {

// A device array of T that frees itself.  Four ways to get memory, each with its own rule for what is there already; none keeps old contents.
// A release in mid-life waits for the handle's stream first (work that reads the array may be pending); the destructor does not wait:
// the destroy function of the handle synchronises once before it deletes the handle.  Moving steals the pointer (a std::vector of them can grow).
template <class T>
struct DevBuf {
  T      *p   = nullptr;
  int64_t cap = 0;  // elements behind p

  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept
  {
    if (this != &o) {
      if (p) (void)hipFree(p);
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { if (p) (void)hipFree(p); }
  operator T *() const { return p; }
  void swap(DevBuf &o) { std::swap(p, o.p), std::swap(cap, o.cap); }
  void release(fl_poisson *h)
  {
    if (p) {
      (void)hipStreamSynchronize(h->stream);
      (void)hipFree(p);
    }
    p   = nullptr;
    cap = 0;
  }
  // at least `need` elements: grown by a quarter beyond the need, never shrunk, zeroed
  int reserve(fl_poisson *h, int64_t need)
  {
    if (p && need <= cap) return 0;
    need = std::max<int64_t>(need + need / 4, 64);
    return exact(h, need, true) ? FL_ERR_MEM : 0;
  }
  // exactly n elements, afresh
  int exact(fl_poisson *h, int64_t n, bool zero)
  {
    release(h);
    const int rc = fl_dev_alloc(h, (void **)&p, sizeof(T) * (size_t)n, zero);
    if (!rc) cap = n;
    return rc;
  }
  // n elements the first time, the same ones ever after
  int once(fl_poisson *h, int64_t n, bool zero) { return p ? 0 : exact(h, n, zero); }
  // exactly n elements by hipMalloc alone -- nothing is written, no stream is involved: a table that a blocking hipMemcpy fills next
  int plain(fl_poisson *h, int64_t n)
  {
    release(h);
    FL_HIP(hipMalloc((void **)&p, sizeof(T) * (size_t)n));
    cap = n;
    return 0;
  }
};

}  // namespace fl

#pragma GCC visibility pop
