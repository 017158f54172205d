// prof.hip — per-kernel HIP-event timing + library-wide entry points.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "common.h"

namespace myslam_hip {

static const char* kNames[P_COUNT] = {"resize", "fast", "octree", "blur7", "describe", "hamming_match", "triangulate",
                                      "lcd_preproc", "calc_conv1", "calc_conv2", "calc_conv3", "lcddb_scan", "ba_build", "screen", "calc_pool2"};
struct Pending { int id; hipEvent_t a, b; };
static std::atomic<bool> g_on{false};
static std::mutex g_mu;
static std::vector<Pending> g_pending;
static std::vector<hipEvent_t> g_pool;
static double g_ms[P_COUNT];
static long g_calls[P_COUNT];
static thread_local hipEvent_t t_start[P_COUNT];

static hipEvent_t get_event() {
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

bool prof_is_on() { return g_on.load(std::memory_order_relaxed); }

void prof_begin(int id, hipStream_t s) {
    if (!g_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_on.load(std::memory_order_relaxed)) return;
    t_start[id] = get_event();
    (void)hipEventRecord(t_start[id], s);
}

void prof_end(int id, hipStream_t s) {
    if (!t_start[id]) return;                 // profiling was off (or switched on mid-call) when the launch began: nothing to pair
    std::lock_guard<std::mutex> lk(g_mu);
    hipEvent_t e = get_event();
    (void)hipEventRecord(e, s);
    g_pending.push_back({id, t_start[id], e});
    t_start[id] = nullptr;
}

// ---- the library's only allocation calls (dev_mem.h) ----
int raw_alloc(void** p, size_t bytes, bool pinned) {
    const hipError_t e = pinned ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes);
    if (e == hipSuccess) return MYSLAM_OK;
    (void)hipGetLastError();                  // the failure is reported here: no later launch check may find it
    fprintf(stderr, "[myslam_hip] %s:%d %s(%zu bytes) -> %s\n", __FILE__, __LINE__, pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
    *p = nullptr;
    return e == hipErrorOutOfMemory ? MYSLAM_ERR_CAPACITY : MYSLAM_ERR_HIP;
}

void raw_free(void* p, bool pinned) {
    if (pinned) (void)hipHostFree(p); else (void)hipFree(p);
}

// ---- thread-local staging of the host-pointer entry points (common.h) ----
void HostArena::release() {
    if (s) (void)hipStreamSynchronize(s);
    m.release();
    if (s) (void)hipStreamDestroy(s);
    s = nullptr;
}

HostArena::~HostArena() { release(); }

int HostArena::open() {
    int cur = 0;
    MYSLAM_HIP_CHECK(hipGetDevice(&cur));
    if (cur != dev) { release(); dev = cur; }          // the calling thread selected another device since its last call
    if (!s) MYSLAM_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return MYSLAM_OK;
}

int HostArena::ensure(size_t dev_bytes, size_t host_bytes) {
    const int rc = open();
    if (rc || m.fits(dev_bytes, host_bytes)) return rc;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return m.grow(dev_bytes, host_bytes);
}

// A device block above 64 MB goes back when its call ends, as it did when every call allocated its own: the general Schur path of the pose graph takes
// gigabytes that nothing else on the thread would use again, and tests/test_gpu_pgo.py holds a thread to 64 MB of device memory across such a call.
void HostArena::trim() {
    if (m.d.size() <= ((size_t)64 << 20)) return;
    if (s) (void)hipStreamSynchronize(s);
    m.d.release();
}

HostArena& host_arena() {
    static thread_local HostArena a;
    return a;
}

hipStream_t host_call_stream() {
    HostArena& a = host_arena();
    if (a.open() == MYSLAM_OK) return a.s;
    (void)hipGetLastError();                           // the caller reports the missing stream: no later launch check may find this
    return nullptr;
}

int HostCall::upload() {
    int rc;
    if ((rc = L.place()) || (rc = A.ensure(L.dev_bytes(), L.host_bytes()))) return rc;
    for (int i = 0; i < L.npc; i++)
        if (L.pc[i].kind <= CallLayout::INOUT && L.pc[i].bytes) memcpy(A.m.h + L.pc[i].off, L.pc[i].src, L.pc[i].bytes);
    if (L.endIn) MYSLAM_HIP_CHECK(hipMemcpyAsync(A.m.d, A.m.h, L.endIn, hipMemcpyHostToDevice, A.s));
    if (L.endZero > L.begZero) MYSLAM_HIP_CHECK(hipMemsetAsync(A.m.d + L.begZero, 0, L.endZero - L.begZero, A.s));
    return MYSLAM_OK;
}

int HostCall::fetch(int piece) {
    const CallLayout::Piece& p = L.pc[piece];
    return copy_sync(A.m.h + p.off, A.m.d + p.off, p.bytes, hipMemcpyDeviceToHost, A.s);
}

int HostCall::download() {
    if (L.endOut > L.begOut) MYSLAM_HIP_CHECK(hipMemcpyAsync(A.m.h + L.begOut, A.m.d + L.begOut, L.endOut - L.begOut, hipMemcpyDeviceToHost, A.s));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(A.s));
    for (int i = 0; i < L.npc; i++)
        if (L.pc[i].kind >= CallLayout::INOUT && L.pc[i].kind <= CallLayout::OUT && L.pc[i].bytes && L.pc[i].dst) memcpy(L.pc[i].dst, A.m.h + L.pc[i].off, L.pc[i].bytes);
    return MYSLAM_OK;
}

static void drain() {
    for (auto& p : g_pending) {
        (void)hipEventSynchronize(p.b);
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { g_ms[p.id] += ms; g_calls[p.id]++; }
        g_pool.push_back(p.a); g_pool.push_back(p.b);
    }
    g_pending.clear();
}

// one wave spins for `ticks` of the constant 100 MHz clock and reports how many SHADER cycles went by: the clock the chip runs at right now
__global__ void k_clock_probe(unsigned long long ticks, unsigned long long* out) {
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_readcyclecounter();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) { __builtin_amdgcn_s_sleep(8); r1 = __builtin_amdgcn_s_memrealtime(); }
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}

}  // namespace myslam_hip

using namespace myslam_hip;

extern "C" {

int myslam_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// build.py passes a digest of every source the library is built from: profiles taken on one build can be told from another's (bench.py: roofline.traffic_stale)
#ifndef MYSLAM_BUILD_ID
#define MYSLAM_BUILD_ID "unidentified"
#endif
const char* myslam_hip_version(void) { return "myslam_hip 0.6 (gfx950) build " MYSLAM_BUILD_ID; }

int myslam_prof_shader_clock_mhz(void* hip_stream, float spin_us, float* mhz) {
    if (!mhz || !(spin_us > 0.f) || spin_us > 1e6f) return MYSLAM_ERR_INVALID;
    static thread_local Buf<unsigned long long> d_t;                  // two counters, allocated once per calling thread
    int rc;
    if (!d_t && (rc = d_t.renew(2))) return rc;
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, (unsigned long long)(spin_us * 100.f), d_t.get());
    MYSLAM_HIP_CHECK(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    MYSLAM_HIP_CHECK(hipMemcpyAsync(h, d_t, 16, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    MYSLAM_HIP_CHECK(hipStreamSynchronize((hipStream_t)hip_stream));
    *mhz = h[1] ? (float)((double)h[0] / (double)h[1] * 100.0) : 0.f;      // shader cycles per 10 ns tick x 100 MHz
    return MYSLAM_OK;
}

int myslam_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!on) drain();
    g_on.store(on != 0);
    return MYSLAM_OK;
}

int myslam_prof_reset(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    drain();
    for (int i = 0; i < P_COUNT; i++) { g_ms[i] = 0; g_calls[i] = 0; }
    return MYSLAM_OK;
}

int myslam_prof_count(void) { return P_COUNT; }

// debug: copy n bytes from a device pointer with this library's HIP runtime (diagnoses runtime/VA mismatches)
int myslam_debug_peek(const void* d_ptr, void* out, size_t n) {
    const hipStream_t st = host_call_stream();          // never the legacy stream (common.h, upload_table)
    return st ? copy_sync(out, d_ptr, n, hipMemcpyDeviceToHost, st) : MYSLAM_ERR_HIP;
}

int myslam_prof_get(int i, const char** name, double* total_ms, long* launches) {
    if (i < 0 || i >= P_COUNT) return MYSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(g_mu);
    drain();
    if (name) *name = kNames[i];
    if (total_ms) *total_ms = g_ms[i];
    if (launches) *launches = g_calls[i];
    return MYSLAM_OK;
}

}  // extern "C"
