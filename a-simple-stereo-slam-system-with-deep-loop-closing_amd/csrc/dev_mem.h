// dev_mem.h — the one owner of device and pinned host memory.  No HIP header: plain C++ (tests/cpp/dev_mem_test.cpp links its own raw_alloc / raw_free).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/myslam_hip.h"

namespace myslam_hip {

// The only callers of the HIP allocation entry points (prof.hip).  raw_alloc -> MYSLAM_OK, MYSLAM_ERR_CAPACITY = out of memory, MYSLAM_ERR_HIP = any other
// failure; a failure is reported on stderr and leaves no sticky HIP error behind.
int raw_alloc(void** p, size_t bytes, bool pinned);
void raw_free(void* p, bool pinned);

// One block of device memory (PINNED: page-locked host memory).  size() is in elements and is 0 whenever the pointer is null, so a guard that reads it never
// passes over a block that a failed growth has freed.  Knows no stream: whoever lets a block move waits for the work that uses it first.
template <class T, bool PINNED = false>
class Buf {
  public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }
    void release() {
        if (p_) raw_free(p_, PINNED);
        p_ = nullptr; n_ = 0;
    }
    // free, then allocate exactly n elements (n == 0 stays empty); `oom_code` is what the caller's entry point reports for out of memory
    int renew(size_t n, int oom_code = MYSLAM_ERR_HIP) {
        release();
        if (n == 0) return MYSLAM_OK;
        void* q = nullptr;
        const int rc = raw_alloc(&q, n * sizeof(T), PINNED);
        if (rc) return rc == MYSLAM_ERR_CAPACITY ? oom_code : rc;
        p_ = static_cast<T*>(q); n_ = n;
        return MYSLAM_OK;
    }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using PinBuf = Buf<T, true>;

// The blocks of one handle whose pointers live in the argument structs of its kernels: own() fills such a pointer by name at the moment its block is
// allocated, so no list of buffers has to be matched to a list of fields.  Destroying the set frees every block it gave out.
class BufSet {
  public:
    // p = a new block of n elements (256 bytes at least), nullptr if it could not be had; -> renew's code
    template <class T>
    int own(T*& p, size_t n, int oom_code = MYSLAM_ERR_HIP) {
        bufs_.emplace_back();
        const int rc = bufs_.back().renew(n * sizeof(T) < 256 ? 256 : n * sizeof(T), oom_code);
        p = reinterpret_cast<T*>(bufs_.back().get());
        return rc;
    }

  private:
    std::vector<Buf<uint8_t>> bufs_;
};

// Growth of a group of buffers guarded by the logical size `cap`: `renews` (-> 0 or the first renew's error) runs with cap == 0, and cap becomes `want`
// only when all of them succeeded — a failed growth leaves a guard that refuses every size.
template <class Cap, class F>
int regrow(Cap& cap, Cap want, F&& renews) {
    cap = 0;
    const int rc = renews();
    if (rc == MYSLAM_OK) cap = want;
    return rc;
}

}  // namespace myslam_hip
