// csrc/dev_mem.h on the host: Buf, BufSet, regrow and the host-pointer calls' staging (CallLayout, ArenaMem) over a malloc-backed raw_alloc / raw_free that
// counts live blocks and can fail the k-th call.
// Built with AddressSanitizer + UBSan by tests/test_dev_mem.py; exit status 0 and "DEV MEM OK" = every check held and nothing leaked.
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "dev_mem.h"

using namespace myslam_hip;

static int g_live = 0, g_peak = 0, g_calls = 0;
static int g_fail_at = 0;                   // > 0: the call with this number (counted from 1 since arm()) fails ...
static int g_fail_code = MYSLAM_ERR_CAPACITY;      // ... with this code
static int g_pinned_live = 0;

static void arm(int k, int code = MYSLAM_ERR_CAPACITY) { g_calls = 0; g_fail_at = k; g_fail_code = code; }

namespace myslam_hip {
int raw_alloc(void** p, size_t bytes, bool pinned) {
    *p = nullptr;
    if (++g_calls == g_fail_at) return g_fail_code;
    *p = malloc(bytes);
    if (!*p) return MYSLAM_ERR_CAPACITY;
    g_live++; g_pinned_live += pinned;
    if (g_live > g_peak) g_peak = g_live;
    return MYSLAM_OK;
}
void raw_free(void* p, bool pinned) {
    free(p);
    g_live--; g_pinned_live -= pinned;
}
}  // namespace myslam_hip

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

template <class B> static bool empty(const B& b) { return b.size() == 0 && b.get() == nullptr; }
template <class B> static bool sound(const B& b) { return b.get() != nullptr || b.size() == 0; }      // never a size over a null pointer

static void single_buffer() {
    Buf<int> b;
    CHECK(empty(b) && g_live == 0);
    arm(0);
    CHECK(b.renew(10) == MYSLAM_OK && b.size() == 10 && b.get() && g_live == 1);
    for (int i = 0; i < 10; i++) b[i] = i;                     // ten whole elements (ASan checks the bytes)
    int* viaConv = b;
    CHECK(viaConv == b.get() && viaConv[9] == 9);
    // renew frees the old block before it asks for the new one: never two live blocks for one buffer
    g_peak = g_live;
    CHECK(b.renew(1000) == MYSLAM_OK && b.size() == 1000 && g_live == 1 && g_peak == 1);
    CHECK(b.renew(3) == MYSLAM_OK && b.size() == 3 && g_live == 1 && g_peak == 1);      // exactly n, also when smaller
    // renew(0) stays empty and asks for nothing
    arm(0);
    CHECK(b.renew(0) == MYSLAM_OK && empty(b) && g_live == 0 && g_calls == 0);
    // release
    CHECK(b.renew(7) == MYSLAM_OK && g_live == 1);
    b.release();
    CHECK(empty(b) && g_live == 0);
    b.release();                                               // twice is harmless
    CHECK(empty(b) && g_live == 0);
    // a failed renew: the old block is gone, and so is the size
    CHECK(b.renew(7) == MYSLAM_OK);
    arm(1);
    CHECK(b.renew(9) == MYSLAM_ERR_HIP && empty(b) && g_live == 0);      // out of memory reports the default oom_code
    arm(0);
    CHECK(b.renew(9) == MYSLAM_OK && b.size() == 9);                     // and the buffer is usable again
    // the oom_code mapping; an error that is not out of memory passes through unchanged
    arm(1);
    CHECK(b.renew(5, MYSLAM_ERR_CAPACITY) == MYSLAM_ERR_CAPACITY && empty(b));
    arm(1, MYSLAM_ERR_HIP);
    CHECK(b.renew(5, MYSLAM_ERR_CAPACITY) == MYSLAM_ERR_HIP && empty(b));
    arm(1, MYSLAM_ERR_INVALID);
    CHECK(b.renew(5) == MYSLAM_ERR_INVALID && empty(b));
    arm(1, MYSLAM_ERR_INVALID);
    CHECK(b.renew(5, MYSLAM_ERR_CAPACITY) == MYSLAM_ERR_INVALID && empty(b));
    arm(0);
    CHECK(g_live == 0);
    // pinned buffers go through the same two functions with the flag set
    {
        PinBuf<double> h;
        CHECK(h.renew(4) == MYSLAM_OK && h.size() == 4 && g_pinned_live == 1 && g_live == 1);
        h[3] = 1.0;
    }
    CHECK(g_live == 0 && g_pinned_live == 0);                  // the destructor frees
}

static void moves() {
    arm(0);
    Buf<char> a;
    CHECK(a.renew(16) == MYSLAM_OK);
    char* const pa = a.get();
    Buf<char> b(std::move(a));
    CHECK(empty(a) && b.get() == pa && b.size() == 16 && g_live == 1);
    Buf<char> c;
    CHECK(c.renew(8) == MYSLAM_OK && g_live == 2);
    c = std::move(b);                                          // frees what c held
    CHECK(empty(b) && c.get() == pa && c.size() == 16 && g_live == 1);
    Buf<char>& self = c;
    c = std::move(self);
    CHECK(c.get() == pa && c.size() == 16 && g_live == 1);
    // into a vector, through its reallocations
    std::vector<Buf<char>> v;
    v.push_back(std::move(c));
    CHECK(empty(c));
    for (int i = 0; i < 20; i++) {
        v.emplace_back();
        CHECK(v.back().renew(i + 1) == MYSLAM_OK);
    }
    CHECK(g_live == 21 && v[0].get() == pa && v[0].size() == 16);
    for (int i = 0; i < 20; i++) CHECK(v[i + 1].size() == (size_t)i + 1 && v[i + 1].get());
    v[5] = std::move(v[20]);
    CHECK(g_live == 20 && empty(v[20]) && v[5].size() == 20);
    v.erase(v.begin());
    CHECK(g_live == 19);
}                                                              // the vector's elements free the rest

struct Group {
    int cap = 0;
    Buf<int> a; Buf<float> b; PinBuf<char> c;
    int grow(int want) {
        return regrow(cap, want, [&]() -> int {
            int rc;
            if ((rc = a.renew(want)) || (rc = b.renew(2 * (size_t)want)) || (rc = c.renew(want + 3, MYSLAM_ERR_CAPACITY))) return rc;
            return MYSLAM_OK;
        });
    }
    bool whole(int want) const { return cap == want && a.size() == (size_t)want && b.size() == 2 * (size_t)want && c.size() == (size_t)want + 3 && a.get() && b.get() && c.get(); }
};

static void groups() {
    for (int k = 1; k <= 3; k++) {
        Group g;
        arm(0);
        CHECK(g.grow(4) == MYSLAM_OK && g.whole(4) && g_live == 3);
        arm(k);                                                // the k-th of the three allocations fails
        const int rc = g.grow(8);
        CHECK(rc == (k == 3 ? MYSLAM_ERR_CAPACITY : MYSLAM_ERR_HIP));
        CHECK(g.cap == 0);                                     // the guard refuses every size, the old one included
        CHECK(sound(g.a) && sound(g.b) && sound(g.c));
        CHECK(g_live == 2);                                    // the one that failed is gone; those before it are new, those behind it still the old ones
        CHECK(k < 2 || g.a.size() == 8);
        CHECK(k < 3 || g.b.size() == 16);
        CHECK((k == 1 ? empty(g.a) : k == 2 ? empty(g.b) : empty(g.c)));
        arm(0);
        CHECK(g.grow(2) == MYSLAM_OK && g.whole(2) && g_live == 3);      // a following growth — a smaller one too — leaves all three whole
        CHECK(g.grow(8) == MYSLAM_OK && g.whole(8) && g_live == 3);
    }
    CHECK(g_live == 0);
    // a step of the group that is no allocation fails (a table upload): the size stays zero as well
    int cap = 5;
    Buf<int> t;
    CHECK(regrow(cap, 9, [&]() -> int { const int rc = t.renew(9); return rc ? rc : MYSLAM_ERR_HIP; }) == MYSLAM_ERR_HIP && cap == 0 && t.size() == 9);
    CHECK(regrow(cap, 9, [&]() -> int { return t.renew(9); }) == MYSLAM_OK && cap == 9);
}

struct Args { double* a = nullptr; int32_t* b = nullptr; uint8_t* c = nullptr; };      // as a kernel's argument struct: filled by member name

static void buf_set() {
    {
        BufSet s;
        Args x;
        arm(0);
        CHECK(s.own(x.a, 100, MYSLAM_ERR_CAPACITY) == MYSLAM_OK && s.own(x.b, 7, MYSLAM_ERR_CAPACITY) == MYSLAM_OK && s.own(x.c, 300) == MYSLAM_OK);
        CHECK(g_live == 3 && x.a && x.b && x.c);
        CHECK((void*)x.a != (void*)x.b && (void*)x.b != (void*)x.c && (void*)x.a != (void*)x.c);
        x.a[99] = 1.0; x.c[299] = 1;                           // whole elements of the asked-for size (ASan checks the bytes)
        for (int i = 0; i < 64; i++) x.b[i] = i;               // 7 x 4 bytes asked for: the block has the floor of 256
        // no element at all still is a block of 256 bytes
        uint8_t* z = nullptr;
        CHECK(s.own(z, 0) == MYSLAM_OK && z && g_live == 4);
        z[0] = 1; z[255] = 2;
        // more blocks than a vector's first capacities: the pointers given out earlier stay what they were
        double* const a0 = x.a;
        for (int i = 0; i < 40; i++) { float* f = nullptr; CHECK(s.own(f, i) == MYSLAM_OK && f); f[63] = 1.0f; }
        CHECK(g_live == 44 && x.a == a0 && x.a[99] == 1.0 && x.b[63] == 63);
    }
    CHECK(g_live == 0);                                        // destroying the set frees every block it gave out
    // the second of three allocations fails: out of memory is the caller's oom_code, any other failure passes through; the pointer is null
    const int codes[2][2] = {{MYSLAM_ERR_CAPACITY, MYSLAM_ERR_UNSUPPORTED}, {MYSLAM_ERR_HIP, MYSLAM_ERR_HIP}};
    for (const auto& c : codes) {
        {
            BufSet s;
            Args x;
            x.b = reinterpret_cast<int32_t*>(&x);              // stale: a failed own must not leave it
            arm(2, c[0]);
            CHECK(s.own(x.a, 10, MYSLAM_ERR_UNSUPPORTED) == MYSLAM_OK && x.a && g_live == 1);
            CHECK(s.own(x.b, 10, MYSLAM_ERR_UNSUPPORTED) == c[1] && x.b == nullptr && g_live == 1);
            CHECK(s.own(x.c, 10, MYSLAM_ERR_UNSUPPORTED) == MYSLAM_OK && x.c && g_live == 2);      // the set stays usable
        }
        CHECK(g_live == 0);
    }
    arm(0);
}

// the staging of the host-pointer calls: where the pieces of a call lie, and what the arena asks the allocator for
static void call_layout() {
    using L = CallLayout;
    // pieces of every kind, registered out of order, some with no byte at all: offsets in the order in, inout, out, zero, tmp, each 256-byte aligned
    L c;
    const int t0 = c.add(L::TMP, nullptr, nullptr, 1000), z0 = c.add(L::ZERO, nullptr, nullptr, 1), o0 = c.add(L::OUT, nullptr, nullptr, 257);
    const int i0 = c.add(L::IN, nullptr, nullptr, 7), io0 = c.add(L::INOUT, nullptr, nullptr, 256), i1 = c.add(L::IN, nullptr, nullptr, 0);
    const int z1 = c.add(L::ZERO, nullptr, nullptr, 0), o1 = c.add(L::OUT, nullptr, nullptr, 0), t1 = c.add(L::TMP, nullptr, nullptr, 0), i2 = c.add(L::IN, nullptr, nullptr, 300);
    const int io1 = c.add(L::INOUT, nullptr, nullptr, 0);
    CHECK(c.place() == MYSLAM_OK && c.npc == 11);
    const int order[11] = {i0, i1, i2, io0, io1, o0, o1, z0, z1, t0, t1};
    size_t off = 0;
    for (int k = 0; k < 11; k++) {
        const L::Piece& p = c.pc[order[k]];
        CHECK(p.off == off && p.off % 256 == 0);
        CHECK(k == 0 || p.kind >= c.pc[order[k - 1]].kind);
        off += (p.bytes + 255) / 256 * 256;
    }
    CHECK(c.pc[i1].off == c.pc[i2].off);                       // a piece of no bytes takes no room
    CHECK(c.begOut == c.pc[io0].off && c.endIn == c.pc[o0].off && c.endOut == c.pc[z0].off && c.begZero == c.endOut);
    CHECK(c.endZero == c.pc[t0].off && c.total == off && c.total == c.pc[t1].off);
    CHECK(c.host_bytes() == c.endOut && c.dev_bytes() == c.total && c.host_bytes() == 256 + 0 + 512 + 256 + 0 + 512 + 0);
    // an empty call and a call of empty pieces
    L e;
    CHECK(e.place() == MYSLAM_OK && e.total == 0 && e.host_bytes() == 0);
    e.add(L::ZERO, nullptr, nullptr, 0); e.add(L::IN, nullptr, nullptr, 0);
    CHECK(e.place() == MYSLAM_OK && e.total == 0 && e.endZero == 0);
    // 1 GB each of zero and tmp beside 1 KB in and out: the pinned block does not know about them
    L g;
    g.add(L::IN, nullptr, nullptr, 512); g.add(L::OUT, nullptr, nullptr, 512); g.add(L::ZERO, nullptr, nullptr, (size_t)1 << 30); g.add(L::TMP, nullptr, nullptr, (size_t)1 << 30);
    CHECK(g.place() == MYSLAM_OK && g.host_bytes() == 1024 && g.host_bytes() < (64u << 10) && g.dev_bytes() == ((size_t)2 << 30) + 1024);
    CHECK(ArenaMem::padded(g.host_bytes()) <= (64u << 10));   // what the arena asks the allocator for: one 64 KB granule
    // MAXP pieces are placed, one more refuses the call (and names piece 0, so that a lookup before place() stays in bounds)
    L f;
    for (int k = 0; k < L::MAXP; k++) CHECK(f.add(L::Kind(k % 5), nullptr, nullptr, k) == k);
    CHECK(L::MAXP == 32 && f.place() == MYSLAM_OK);
    CHECK(f.add(L::TMP, nullptr, nullptr, 8) == 0 && f.npc == L::MAXP && f.place() == MYSLAM_ERR_CAPACITY);
}

static void arena_mem() {
    arm(0);
    {
        ArenaMem m;
        CHECK(!m.fits(0, 0));                                  // no block yet: not even an empty call fits
        CHECK(m.grow(0, 0) == MYSLAM_OK && m.fits(0, 0) && m.d.size() >= 256 && m.h.size() >= 256 && g_live == 2 && g_pinned_live == 1);
        m.d[m.d.size() - 1] = 1; m.h[m.h.size() - 1] = 1;      // whole blocks (ASan checks the bytes)
        // the device side grows alone: the pinned block stays the one it was
        uint8_t* const h0 = m.h.get();
        const size_t hs = m.h.size();
        CHECK(!m.fits(1 << 20, 100) && m.grow(1 << 20, 100) == MYSLAM_OK && m.fits(1 << 20, 100) && m.h.get() == h0 && m.h.size() == hs && g_live == 2);
        CHECK(m.d.size() >= (1 << 20) + (1 << 18));            // a quarter of headroom
        uint8_t* const d0 = m.d.get();
        CHECK(m.grow(1000, hs + 1) == MYSLAM_OK && m.d.get() == d0 && m.h.size() > hs);      // and the pinned side alone; nothing shrinks
        // a failed growth, of either block, leaves both sizes 0 and nothing live
        for (int k = 1; k <= 2; k++) {
            CHECK(m.grow(1, 1) == MYSLAM_OK && g_live == 2);
            arm(k);
            CHECK(m.grow(m.d.size() + 1, m.h.size() + 1) == MYSLAM_ERR_HIP);
            CHECK(empty(m.d) && empty(m.h) && !m.fits(0, 0) && g_live == 0);
            arm(0);
        }
        CHECK(m.grow(1, 1) == MYSLAM_OK && g_live == 2);
        arm(1);                                                // only the pinned block is short, and its growth fails: the device block goes too
        CHECK(m.grow(1, m.h.size() + 1) == MYSLAM_ERR_HIP && empty(m.d) && empty(m.h) && g_live == 0);
        arm(0);
        CHECK(m.grow(1, 1) == MYSLAM_OK && m.fits(1, 1));       // usable again
    }
    CHECK(g_live == 0 && g_pinned_live == 0);
}

int main() {
    call_layout();
    arena_mem();
    CHECK(g_live == 0);
    single_buffer();
    CHECK(g_live == 0);
    moves();
    CHECK(g_live == 0);
    groups();
    CHECK(g_live == 0);
    buf_set();
    CHECK(g_live == 0 && g_pinned_live == 0);
    printf("DEV MEM OK\n");
    return 0;
}
