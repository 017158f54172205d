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

// ---- the host-pointer entry points' staging, the part that needs no HIP call (HostCall and HostArena, common.h, put the copies and the stream on top) ----
// The pieces of one call, each 256-byte aligned, laid out by kind: [in][inout][out][zero][tmp].  [0, endIn) goes up in one copy, [begOut, endOut) comes back
// in one, [begZero, endZero) is cleared by one memset, TMP is whatever an earlier call left there.  Only [0, endOut) has a pinned mirror.
class CallLayout {
  public:
    enum Kind { IN = 0, INOUT = 1, OUT = 2, ZERO = 3, TMP = 4 };
    static constexpr int MAXP = 32;
    struct Piece { Kind kind; const void* src; void* dst; size_t bytes, off; };

    // -> the piece's number; past MAXP pieces place() refuses the call, and piece 0 keeps every offset lookup in bounds until then
    int add(Kind k, const void* src, void* dst, size_t bytes) {
        if (npc >= MAXP) { overflow = true; return 0; }
        pc[npc] = {k, src, dst, bytes, 0};
        return npc++;
    }
    int place() {
        if (overflow) return MYSLAM_ERR_CAPACITY;
        size_t off = 0;
        for (int k = IN; k <= TMP; k++) {
            if (k == INOUT) begOut = off;
            if (k == ZERO) begZero = off;
            for (int i = 0; i < npc; i++)
                if (pc[i].kind == k) { pc[i].off = off; off += (pc[i].bytes + 255) & ~(size_t)255; }
            if (k == INOUT) endIn = off;
            if (k == OUT) endOut = off;
            if (k == ZERO) endZero = off;
        }
        total = off;
        return MYSLAM_OK;
    }
    size_t host_bytes() const { return endOut; }       // the pinned block mirrors what is copied, never ZERO or TMP
    size_t dev_bytes() const { return total; }

    Piece pc[MAXP];
    int npc = 0;
    bool overflow = false;
    size_t endIn = 0, begOut = 0, endOut = 0, begZero = 0, endZero = 0, total = 0;
};

// The two blocks of a staging arena.  Grow-only, each by its own need; a failed growth frees both, so neither size outlives its block's partner.
struct ArenaMem {
    Buf<uint8_t> d; PinBuf<uint8_t> h;
    bool fits(size_t dev_bytes, size_t host_bytes) const { return d && h && dev_bytes <= d.size() && host_bytes <= h.size(); }
    // whoever calls this has waited for the work that uses the blocks
    int grow(size_t dev_bytes, size_t host_bytes) {
        int rc = MYSLAM_OK;
        if (!d || d.size() < dev_bytes) rc = d.renew(padded(dev_bytes));
        if (!rc && (!h || h.size() < host_bytes)) rc = h.renew(padded(host_bytes));
        if (rc) release();
        return rc;
    }
    void release() { d.release(); h.release(); }
    static size_t padded(size_t bytes) { return (bytes + (bytes >> 2) + 65536) & ~(size_t)65535; }      // a quarter of headroom, whole 64 KB, never nothing
};

}  // namespace myslam_hip
