// owned_buf.h — a move-only owner of one allocation: pointer + capacity in elements.  Host-only and runtime-free: the Policy supplies
// `static E alloc(void** p, size_t bytes)` (E: an error code, E{} = success) and `static void release(void* p)`.  capi_internal.h defines
// the device and pinned-host policies; tests/test_owned_buf_cpu.py drives it with a malloc policy under ASan + UBSan.
#pragma once
#include <stddef.h>

namespace slam_host {

template <class T, class Policy>
class Buf {
  public:
    using error_t = decltype(Policy::alloc((void**)nullptr, (size_t)0));
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~Buf() { reset(); }

    // room for at least n elements.  The new block is allocated BEFORE the old one is released, so a failure returns the error and
    // leaves the old block and its capacity as they were.  Contents are not preserved.
    error_t reserve(size_t n) {
        if (n <= n_) return error_t{};
        void* q = nullptr;
        const error_t e = Policy::alloc(&q, sizeof(T) * n);
        if (e != error_t{}) return e;
        reset();
        p_ = static_cast<T*>(q); n_ = n;
        return error_t{};
    }
    void reset() { if (p_) Policy::release(p_); p_ = nullptr; n_ = 0; }
    T* get() const { return p_; }
    size_t cap() const { return n_; }
    operator T*() const { return p_; }   // reads like the raw pointer it replaces (kernel parameters, offsets, null tests)

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace slam_host
