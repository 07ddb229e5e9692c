// lcs_mem.h -- the one owner of every block of device, page-locked and staging memory a context holds (included by
// lcs_internal.h).  A Buf is move-only, frees its block exactly once (reset(), a later alloc(), or its destructor) and
// carries its capacity in elements: the capacity is non-zero only while the block it describes exists, so a failed
// alloc() / reserve() leaves an empty owner that the next call allocates again.  It converts to T * by itself, so that
// kernel arguments, copy operands, pointer arithmetic and `if (c->xcb.btab)` read as they do with a raw pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdlib>
#include "../../include/lcs.h"

struct lcs_ctx;
int lcs_hip_error(lcs_ctx *c, const char *call, hipError_t e);   // lcs_internal.h: c->err = "<call>: <HIP's text>", returns LCS_ERR_HIP

struct LcsDeviceMem {
  static constexpr const char *name = "hipMalloc";
  static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void put(void *p) { (void)hipFree(p); }
};
struct LcsPinnedMem {
  static constexpr const char *name = "hipHostMalloc";
  static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void put(void *p) { (void)hipHostFree(p); }
};
struct LcsPageableMem {      // ordinary host memory (the tracker's staging block: tracker.hip says why it is not page-locked)
  static constexpr const char *name = "malloc";
  static hipError_t get(void **p, size_t bytes) { return (*p = std::malloc(bytes)) ? hipSuccess : hipErrorOutOfMemory; }
  static void put(void *p) { std::free(p); }
};

template <typename T, typename Mem>
class Buf {
 public:
  Buf() = default;
  Buf(Buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~Buf() { reset(); }

  // A block of exactly n elements.  The old block goes FIRST (the peak never holds both); n == 0 leaves the owner empty.
  // The caller has synchronised whatever may still read the old block.
  int alloc(lcs_ctx *c, size_t n) {
    reset();
    if (n == 0) return LCS_OK;
    void *p = nullptr;
    const hipError_t e = Mem::get(&p, n * sizeof(T));
    if (e != hipSuccess) return lcs_hip_error(c, Mem::name, e);
    p_ = static_cast<T *>(p);
    n_ = n;
    return LCS_OK;
  }
  // Grow only: the block stays when it already holds n elements.
  int reserve(lcs_ctx *c, size_t n) { return n <= n_ ? LCS_OK : alloc(c, n); }
  void reset() {
    if (p_) Mem::put(p_);
    p_ = nullptr;
    n_ = 0;
  }
  T *get() const { return p_; }
  size_t capacity() const { return n_; }
  operator T *() const { return p_; }

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
};
template <typename T> using DevBuf = Buf<T, LcsDeviceMem>;
template <typename T> using PinnedBuf = Buf<T, LcsPinnedMem>;
