// lcd_bank.hip — S loop databases in one device allocation, scanned and appended on the device (gfx950).
// A bank of S streams is S reference Systems, hence S LoopClosing::_mvDatabase maps (include/myslam/loopclosing.h:120) whose key-frame ids all start at 0.
// Replaces, per stream, the gate of LoopClosingRun (src/loopclosing.cpp:62), DetectLoop's scan (:126-143) and AddToDatabase (:651-659).
//
// HBM layout, fixed at create: rows [S][rows_per_stream][1064] f32 (4256-byte rows, 16-byte aligned), ids [S][rows_per_stream] u64 ascending per stream,
// count [S] i32.  Ids, counts and row limits never visit the host: a recorded step that names the bank stays valid, and a replay sees later appends.
//
// A query is three dependent launches on the handle's stream:
//   k_bank_limits   one workgroup per stream: idle / gate / the first row inside the cut-off window (:133) -> lim[s], d_status[s]
//   k_bank_scan     grid (row tiles, S): a workgroup whose tile lies at or behind lim[s] returns after reading lim[s]; else one wave per row, the
//                   stream's query in registers, 16-byte loads, one partial (score, row, cnt) per tile into handle-owned scratch
//   k_bank_reduce   one wave per stream over the partials of the tiles below lim[s] -> the five outputs
// No flags, no atomics, no hand-off inside a launch.  The scan is HBM-bound: every row below a limit is read once (4256 B), the query once per wave
// from L2.
#include <algorithm>

#include "common.h"

namespace myslam_hip {

constexpr int BK_DIM = MYSLAM_LCD_DIM;                  // 1064 floats = 266 float4 = 4 x 64 + 10
constexpr int BK_VEC = BK_DIM / 4;                      // 266
constexpr int BK_TAIL = BK_VEC - 4 * WAVE;              // 10 lanes hold a fifth float4
constexpr int BK_WAVES = 4;
constexpr int BK_ROWS_PER_WAVE = MYSLAM_LCDBANK_ROW_TILE / BK_WAVES;
constexpr int BK_TILE = MYSLAM_LCDBANK_ROW_TILE;        // rows per workgroup
static_assert(BK_DIM % 4 == 0 && BK_TAIL > 0 && BK_TAIL <= WAVE && BK_TILE == BK_WAVES * BK_ROWS_PER_WAVE, "row layout");

struct BankPartial { float score; int32_t row; int32_t cnt; };

struct BankView {
    float* rows; uint64_t* ids; int32_t* n;
    int S, rps;
};

__device__ __forceinline__ int bank_count(const BankView& v, int s) { return min(max(v.n[s], 0), v.rps); }

// lim[s] = rows the scan of stream s walks: 0 for an idle or gated item, else the index of the first row with (cur - id) mod 2^64 < 20 (the count when
// there is none).  Every row's id is tested, so the window that wraps for cur < 19 needs no case of its own.
__global__ __launch_bounds__(256) void k_bank_limits(BankView v, const uint64_t* __restrict__ cur_id, const int32_t* __restrict__ active, int min_size,
                                                     int32_t* __restrict__ lim, int32_t* __restrict__ status) {
    __shared__ int s_first[BK_WAVES];
    const int s = blockIdx.x, t = threadIdx.x;
    if (active && active[s] == 0) {                                     // (uniform per block: nothing of the item's inputs is read)
        if (t == 0) { lim[s] = 0; status[s] = MYSLAM_LCDBANK_IDLE; }
        return;
    }
    const int n = bank_count(v, s);
    if (n <= min_size) {                                                // _mvDatabase.size() > _mnDatabaseMinSize, loopclosing.cpp:62
        if (t == 0) { lim[s] = 0; status[s] = MYSLAM_LCDBANK_GATED; }
        return;
    }
    const uint64_t cur = cur_id[s];
    const uint64_t* ids = v.ids + (size_t)s * v.rps;
    int first = n;
    for (int r = t; r < n; r += 256)
        if (cur - ids[r] < 20) { first = r; break; }                    // unsigned: loopclosing.cpp:133
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if ((t & 63) == 0) s_first[t >> 6] = first;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < BK_WAVES; w++) first = min(first, s_first[w]);
        lim[s] = first; status[s] = MYSLAM_LCDBANK_SCANNED;
    }
}

// One wave per row.  A lane's products are added in one chain (float4 k = 0 .. 3: x, y, z, w; then the tail's), the 64 lane sums by the __shfl_xor
// butterfly: the order depends on nothing but the position of an entry inside its row.
__global__ __launch_bounds__(256) void k_bank_scan(BankView v, const float* __restrict__ q, const int32_t* __restrict__ lim, float thr_low,
                                                   BankPartial* __restrict__ partials, int ntiles) {
    __shared__ BankPartial s_p[BK_WAVES];
    const int s = blockIdx.y, tile = blockIdx.x;
    const int L = min(lim[s], v.rps);
    const int r0 = tile * BK_TILE;
    if (r0 >= L) return;                                                // behind the limit: nothing else is read, and k_bank_reduce skips the slot
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float4* q4 = reinterpret_cast<const float4*>(q + (size_t)s * BK_DIM);
    float4 qv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) qv[k] = q4[k * WAVE + lane];
    const float4 qt = lane < BK_TAIL ? q4[4 * WAVE + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float* base = v.rows + (size_t)s * v.rps * BK_DIM;
    float bs = 0.f; int bi = -1, cnt = 0;
    const int rw = r0 + wave * BK_ROWS_PER_WAVE;
    const int rend = min(rw + BK_ROWS_PER_WAVE, L);                     // rows at or above the limit are not read
    for (int r = rw; r < rend; r++) {
        const float4* row = reinterpret_cast<const float4*>(base + (size_t)r * BK_DIM);
        float4 a[4];
#pragma unroll
        for (int k = 0; k < 4; k++) a[k] = row[k * WAVE + lane];
        const float4 at = lane < BK_TAIL ? row[4 * WAVE + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) { acc += a[k].x * qv[k].x; acc += a[k].y * qv[k].y; acc += a[k].z * qv[k].z; acc += a[k].w * qv[k].w; }
        if (lane < BK_TAIL) { acc += at.x * qt.x; acc += at.y * qt.y; acc += at.z * qt.z; acc += at.w * qt.w; }
        acc = wave_reduce_sum(acc);
        if (acc > bs) { bs = acc; bi = r; }                             // rows ascend: strict '>' keeps the lowest; NaN compares false
        cnt += (acc > thr_low) ? 1 : 0;
    }
    if (lane == 0) s_p[wave] = {bs, bi, cnt};
    __syncthreads();
    if (threadIdx.x == 0) {
        BankPartial best = s_p[0];
        for (int w = 1; w < BK_WAVES; w++) {                            // waves own ascending row ranges
            const BankPartial p = s_p[w];
            if (p.score > best.score) { best.score = p.score; best.row = p.row; }
            best.cnt += p.cnt;
        }
        partials[(size_t)s * ntiles + tile] = best;
    }
}

// One wave per stream, k_db_reduce's merge (lcddb.hip): lanes take the tiles lane, lane + 64, ... in ascending order, then the 64 candidates are merged —
// larger score wins, equal scores -> lower row.  Only the tiles below the limit hold a partial of this call.
__global__ __launch_bounds__(256) void k_bank_reduce(BankView v, const BankPartial* __restrict__ partials, int ntiles, const int32_t* __restrict__ lim,
                                                     uint64_t* __restrict__ best_id, float* __restrict__ max_score, int32_t* __restrict__ cnt,
                                                     int32_t* __restrict__ best_row) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= v.S) return;
    const int L = min(lim[s], v.rps);
    const int nt = (L + BK_TILE - 1) / BK_TILE;
    float ms = 0.f; int bi = -1; int c = 0;
    for (int b = lane; b < nt; b += 64) {
        const BankPartial p = partials[(size_t)s * ntiles + b];
        if (p.score > ms) { ms = p.score; bi = p.row; }
        c += p.cnt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(ms, o, 64); const int oi = __shfl_xor(bi, o, 64);
        c += __shfl_xor(c, o, 64);
        if (os > ms || (os == ms && oi >= 0 && (bi < 0 || oi < bi))) { ms = os; bi = oi; }
    }
    if (lane == 0) {
        best_id[s] = (bi >= 0) ? v.ids[(size_t)s * v.rps + bi] : 0;     // bestId initialised to 0, loopclosing.cpp:129
        max_score[s] = ms; cnt[s] = c; best_row[s] = bi;
    }
}

// AddToDatabase (:651-659), one workgroup per stream: everything is decided from the count read at entry, the row and the id land at that slot, the
// count moves last.
__global__ __launch_bounds__(256) void k_bank_append(BankView v, const float* __restrict__ descr, const uint64_t* __restrict__ id,
                                                     const int32_t* __restrict__ add, int32_t* __restrict__ status) {
    const int s = blockIdx.x, t = threadIdx.x;
    if (add && add[s] == 0) {
        if (t == 0) status[s] = MYSLAM_LCDBANK_IDLE;
        return;
    }
    const int raw = v.n[s];
    const int n = min(max(raw, 0), v.rps);
    int st = MYSLAM_LCDBANK_ADDED;
    if (n >= v.rps) st = MYSLAM_ERR_CAPACITY;
    else if (n > 0 && id[s] <= v.ids[(size_t)s * v.rps + n - 1]) st = MYSLAM_ERR_INVALID;      // std::map order: ids ascend strictly
    if (st == MYSLAM_LCDBANK_ADDED) {                                   // (uniform per block)
        float* dst = v.rows + ((size_t)s * v.rps + n) * BK_DIM;
        const float* src = descr + (size_t)s * BK_DIM;
        for (int k = t; k < BK_DIM; k += 256) dst[k] = src[k];
    }
    __syncthreads();                                                    // every thread has read the count before it moves
    if (t == 0) {
        if (st == MYSLAM_LCDBANK_ADDED) { v.ids[(size_t)s * v.rps + n] = id[s]; v.n[s] = n + 1; }
        status[s] = st;
    }
}

__global__ __launch_bounds__(256) void k_bank_clear(BankView v, const int32_t* __restrict__ clear) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < v.S && clear[s] != 0) v.n[s] = 0;
}

}  // namespace myslam_hip

using namespace myslam_hip;

// Nothing here changes after create but the stream: the calls below are launches over fixed pointers.
struct myslam_lcdbank {
    hipStream_t stream = nullptr;
    BankView v{};
    int ntiles = 0;
    BankPartial* d_partials = nullptr;      // [S][ntiles]
    int32_t* d_lim = nullptr;               // [S]
    BufSet mem;
};

static int bank_sync(const myslam_lcdbank* h) {
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    return MYSLAM_OK;
}

static int bank_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    const hipStream_t st = host_call_stream();
    if (!st) return MYSLAM_ERR_HIP;
    return copy_sync(dst, src, bytes, kind, st);
}

extern "C" {

int myslam_lcdbank_create(myslam_lcdbank** out, int streams, int rows_per_stream) {
    if (!out || streams <= 0 || rows_per_stream <= 0) return MYSLAM_ERR_INVALID;
    if (streams > 65535 || rows_per_stream > (1 << 24)) return MYSLAM_ERR_CAPACITY;      // grid.y / one launch covers a stream's tiles
    if (need_device()) return MYSLAM_ERR_HIP;
    myslam_lcdbank* h = new myslam_lcdbank();
    h->v.S = streams; h->v.rps = rows_per_stream;
    h->ntiles = (rows_per_stream + BK_TILE - 1) / BK_TILE;
    const size_t S = (size_t)streams, R = (size_t)rows_per_stream;
    int rc;
    if ((rc = h->mem.own(h->v.rows, S * R * BK_DIM, MYSLAM_ERR_CAPACITY)) || (rc = h->mem.own(h->v.ids, S * R, MYSLAM_ERR_CAPACITY)) ||
        (rc = h->mem.own(h->v.n, S, MYSLAM_ERR_CAPACITY)) || (rc = h->mem.own(h->d_partials, S * h->ntiles, MYSLAM_ERR_CAPACITY)) ||
        (rc = h->mem.own(h->d_lim, S, MYSLAM_ERR_CAPACITY))) {
        delete h;
        return rc;
    }
    auto zero_all = [&]() -> int {      // every stream starts empty; rows and ids read the same on every run (never the legacy stream, common.h)
        const hipStream_t us = host_call_stream();
        if (!us) return MYSLAM_ERR_HIP;
        MYSLAM_HIP_CHECK(hipMemsetAsync(h->v.rows, 0, S * R * BK_DIM * sizeof(float), us));
        MYSLAM_HIP_CHECK(hipMemsetAsync(h->v.ids, 0, S * R * sizeof(uint64_t), us));
        MYSLAM_HIP_CHECK(hipMemsetAsync(h->v.n, 0, S * sizeof(int32_t), us));
        MYSLAM_HIP_CHECK(hipMemsetAsync(h->d_lim, 0, S * sizeof(int32_t), us));
        MYSLAM_HIP_CHECK(hipStreamSynchronize(us));
        return MYSLAM_OK;
    };
    if ((rc = zero_all())) { delete h; return rc; }
    *out = h;
    return MYSLAM_OK;
}

int myslam_lcdbank_destroy(myslam_lcdbank* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_lcdbank_set_stream(myslam_lcdbank* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    return MYSLAM_OK;
}

int myslam_lcdbank_row_tile(void) { return BK_TILE; }

int myslam_lcdbank_launches_per_query(void) { return 3; }

int myslam_lcdbank_query_batch(myslam_lcdbank* h, const float* d_q, const uint64_t* d_cur_id, const int32_t* d_active, float thr_low, int min_size,
                               uint64_t* d_best_id, float* d_max_score, int32_t* d_cnt, int32_t* d_best_row, int32_t* d_status) {
    if (!h || !d_q || !d_cur_id || !d_best_id || !d_max_score || !d_cnt || !d_best_row || !d_status) return MYSLAM_ERR_INVALID;
    if ((uintptr_t)d_q & 15) return MYSLAM_ERR_INVALID;                 // the scan reads the queries with 16-byte loads
    const BankView& v = h->v;
    hipLaunchKernelGGL(k_bank_limits, dim3(v.S), dim3(256), 0, h->stream, v, d_cur_id, d_active, min_size, h->d_lim, d_status);
    {
        ScopedProf sp(P_DBSCAN, h->stream);
        hipLaunchKernelGGL(k_bank_scan, dim3(h->ntiles, v.S), dim3(256), 0, h->stream, v, d_q, h->d_lim, thr_low, h->d_partials, h->ntiles);
    }
    hipLaunchKernelGGL(k_bank_reduce, dim3((v.S + 3) / 4), dim3(256), 0, h->stream, v, h->d_partials, h->ntiles, h->d_lim, d_best_id, d_max_score, d_cnt,
                       d_best_row);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_lcdbank_append_batch(myslam_lcdbank* h, const float* d_descr, const uint64_t* d_id, const int32_t* d_add, int32_t* d_status) {
    if (!h || !d_descr || !d_id || !d_status) return MYSLAM_ERR_INVALID;
    hipLaunchKernelGGL(k_bank_append, dim3(h->v.S), dim3(256), 0, h->stream, h->v, d_descr, d_id, d_add, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_lcdbank_clear_batch(myslam_lcdbank* h, const int32_t* d_clear) {
    if (!h || !d_clear) return MYSLAM_ERR_INVALID;
    hipLaunchKernelGGL(k_bank_clear, dim3((h->v.S + 255) / 256), dim3(256), 0, h->stream, h->v, d_clear);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_lcdbank_view(const myslam_lcdbank* h, const float** d_rows, const uint64_t** d_ids, const int32_t** d_n) {
    if (!h || !d_rows || !d_ids || !d_n) return MYSLAM_ERR_INVALID;
    *d_rows = h->v.rows; *d_ids = h->v.ids; *d_n = h->v.n;
    return MYSLAM_OK;
}

int myslam_lcdbank_load(myslam_lcdbank* h, int s, const uint64_t* ids, const float* rows, int n) {
    if (!h || s < 0 || s >= h->v.S || n < 0 || (n > 0 && (!ids || !rows))) return MYSLAM_ERR_INVALID;
    if (n > h->v.rps) return MYSLAM_ERR_CAPACITY;
    for (int i = 1; i < n; i++)
        if (ids[i] <= ids[i - 1]) return MYSLAM_ERR_INVALID;
    int rc;
    if ((rc = bank_sync(h))) return rc;
    const size_t at = (size_t)s * h->v.rps;
    const int32_t cnt = n;
    if (n && ((rc = bank_copy(h->v.rows + at * BK_DIM, rows, (size_t)n * BK_DIM * sizeof(float), hipMemcpyHostToDevice)) ||
              (rc = bank_copy(h->v.ids + at, ids, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice))))
        return rc;
    return bank_copy(h->v.n + s, &cnt, sizeof(cnt), hipMemcpyHostToDevice);
}

int myslam_lcdbank_get(myslam_lcdbank* h, int s, uint64_t* ids, float* rows, int cap, int* n) {
    if (!h || s < 0 || s >= h->v.S || cap < 0 || !n) return MYSLAM_ERR_INVALID;
    int rc;
    if ((rc = bank_sync(h))) return rc;
    int32_t cnt = 0;
    if ((rc = bank_copy(&cnt, h->v.n + s, sizeof(cnt), hipMemcpyDeviceToHost))) return rc;
    cnt = std::min(std::max(cnt, 0), h->v.rps);
    *n = cnt;
    if (cnt > cap) return MYSLAM_ERR_CAPACITY;
    const size_t at = (size_t)s * h->v.rps;
    if (cnt && ids && (rc = bank_copy(ids, h->v.ids + at, (size_t)cnt * sizeof(uint64_t), hipMemcpyDeviceToHost))) return rc;
    if (cnt && rows && (rc = bank_copy(rows, h->v.rows + at * BK_DIM, (size_t)cnt * BK_DIM * sizeof(float), hipMemcpyDeviceToHost))) return rc;
    return MYSLAM_OK;
}

int myslam_lcdbank_sizes(myslam_lcdbank* h, int32_t* n) {
    if (!h || !n) return MYSLAM_ERR_INVALID;
    int rc;
    if ((rc = bank_sync(h))) return rc;
    if ((rc = bank_copy(n, h->v.n, (size_t)h->v.S * sizeof(int32_t), hipMemcpyDeviceToHost))) return rc;
    for (int s = 0; s < h->v.S; s++) n[s] = std::min(std::max(n[s], 0), h->v.rps);
    return MYSLAM_OK;
}

}  // extern "C"
