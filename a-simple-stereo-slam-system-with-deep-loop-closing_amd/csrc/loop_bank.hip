// loop_bank.hip — S per-stream loop key-frame stores in device memory (gfx950), with the three decisions of LoopClosingRun (src/loopclosing.cpp:51-80)
// that lie between the batched units taken on the device: which key-frames the loop closer takes at all (LoopClosing::InsertNewKeyFrame, :671-681),
// which ones end unconfirmed and are kept (:73-75, AddToDatabase's store half, :651-659) and _mpLastClosedKF (:331).  A bank of S streams is S reference
// Systems: S _mvDatabase maps whose ids all start at 0, S _mpLastClosedKF.
//
// HBM layout, fixed at create (K key-frames per stream, strides rounded to 4 as in loop_store.hip): key-points [S][K][cap_st], descriptors
// [S][K][cap_st x 32], landmark tables [S][K][feat_st], rows / nfeat [S][K] i32, ids [S][K] u64 ascending per stream, n [S] i32, last_closed [S] i64
// (-1 = none), put_slot [S] i32.  Ids, counts and last_closed never visit the host: a recorded step that names the bank stays valid, and a replay sees
// what was stored after the recording.  A stream of the bank is an LsStore (loop_store_view.h) whose pointers are offset to the stream and whose size
// is &n[s]: the copies, the clamps, the chunking and the walk of set_links are the store's own code.
//
//   k_lbank_gate     a thread per stream: InsertNewKeyFrame's unsigned expression -> d_active, d_status
//   k_lbank_detect   grid (chunks, S): k_loop_detect's decision; the lookup is ONE load, ids[s][d_best_row[s]] against d_best_id[s]; then the gather
//   k_lbank_plan     one workgroup, a thread per stream: idle / closed (last_closed moves) / full / id not ascending / stored -> put_slot[s], d_add, d_status
//   k_lbank_put      grid (chunks, S): a workgroup reads put_slot[s] and returns when it is -1, else moves its share of the item into that slot; chunk 0
//                    writes rows, nfeat, the id and n[s] = put_slot[s] + 1.  Nothing in this launch reads n[s] or writes put_slot[s]: the count changes at
//                    the launch boundary, so there is no flag, atomic or fence inside a launch.
//   k_lbank_links    a workgroup per stream: ls_walk_links over the stream's ids
//   k_lbank_clear    a thread per stream
// Every decision is wave-uniform and repeated per workgroup; the copies are bandwidth kernels, 16 bytes per lane where both sides of an item are aligned.
#include "loop_store_view.h"

namespace myslam_hip {

struct LbBank {
    myslam_keypoint* kps; uint8_t* desc; int32_t* lm;
    int32_t* rows; int32_t* nfeat; uint64_t* ids; int32_t* n; int64_t* last_closed; int32_t* put_slot;
    int S, K, cap, feat_cap; size_t cap_st, feat_st;
};

// stream s as a store of K slots
__device__ __forceinline__ LsStore lb_stream(const LbBank& b, int s) {
    const size_t at = (size_t)s * b.K;
    return LsStore{b.kps + at * b.cap_st, b.desc + at * b.cap_st * 32, b.lm + at * b.feat_st, b.rows + at, b.nfeat + at, b.ids + at, b.n + s,
                   b.cap, b.feat_cap, b.cap_st, b.feat_st};
}

// InsertNewKeyFrame (:671-681): `_mpLastClosedKF == nullptr || pNewKF->mnKFId - _mpLastClosedKF->mnKFId > 5`, unsigned long arithmetic
__global__ void __launch_bounds__(LS_THREADS) k_lbank_gate(const LbBank bk, const int64_t* __restrict__ new_kf_id, const int32_t* __restrict__ item_status,
                                                           int status_stride, int32_t* __restrict__ active, int32_t* __restrict__ status) {
    const int s = blockIdx.x * LS_THREADS + threadIdx.x;
    if (s >= bk.S) return;
    const int64_t id = new_kf_id[s];
    int st = MYSLAM_LOOP_BANK_IDLE;
    if (id >= 0 && (!item_status || item_status[(size_t)s * status_stride] == 0)) {
        const int64_t last = bk.last_closed[s];
        st = (last < 0 || (uint64_t)id - (uint64_t)last > 5) ? MYSLAM_LOOP_BANK_TURN : MYSLAM_LOOP_BANK_SKIPPED;
    }
    active[s] = st == MYSLAM_LOOP_BANK_TURN ? 1 : 0;
    status[s] = st;
}

// detect: the decision of loopclosing.cpp:147 per stream, `_mvDatabase.at(bestId)` (:151) as the row the scan found, then the gather
__global__ void __launch_bounds__(LS_THREADS) k_lbank_detect(const LbBank bk, const uint64_t* __restrict__ best_id, const int32_t* __restrict__ best_row,
                                                             const float* __restrict__ max_score, const int32_t* __restrict__ cnt, float thr_high,
                                                             int max_suspected, uint8_t* __restrict__ loop_desc, int32_t* __restrict__ n_loop,
                                                             myslam_keypoint* __restrict__ loop_pyr, int32_t* __restrict__ loop_lm,
                                                             int32_t* __restrict__ loop_slot, int32_t* __restrict__ status) {
    const int s = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const bool lead = chunk == 0 && threadIdx.x == 0;
    // the reference's expression as written: a NaN score is not "less" and goes on to the lookup
    if (max_score[s] < thr_high || cnt[s] > max_suspected) {
        if (lead) { status[s] = MYSLAM_LOOP_DETECT_NO_LOOP; n_loop[s] = 0; loop_slot[s] = -1; }
        return;
    }
    const LsStore st = lb_stream(bk, s);
    const int held = ls_clamp(*st.size, bk.K);
    const int row = best_row[s];
    if (row < 0 || row >= held || st.ids[row] != best_id[s]) {
        if (lead) { status[s] = MYSLAM_ERR_INVALID; n_loop[s] = 0; loop_slot[s] = -1; }
        return;
    }
    const size_t slot = (size_t)row;
    const int n = ls_clamp(st.rows[slot], st.cap), nf = ls_clamp(st.nfeat[slot], st.feat_cap);
    if (lead) { status[s] = MYSLAM_LOOP_DETECT_CANDIDATE; n_loop[s] = n; loop_slot[s] = row; }
    ls_copy(loop_pyr + (size_t)s * st.cap, st.kps + slot * st.cap_st, (size_t)n * LS_KP_BYTES, chunk, nchunks);
    ls_copy(loop_desc + (size_t)s * st.cap * 32, st.desc + slot * st.cap_st * 32, (size_t)n * 32, chunk, nchunks);
    ls_copy(loop_lm + (size_t)s * st.feat_cap, st.lm + slot * st.feat_st, (size_t)nf * 4, chunk, nchunks);
}

// finish, launch a: `if(!bConfirmedLoopKF) AddToDatabase()` (:73-75) and `_mpLastClosedKF = _mpCurrentKF` (:331) per stream
__global__ void __launch_bounds__(LS_THREADS) k_lbank_plan(const LbBank bk, const uint64_t* __restrict__ cur_id, const int32_t* __restrict__ active,
                                                           const int32_t* __restrict__ verify_status, int32_t* __restrict__ add,
                                                           int32_t* __restrict__ status) {
    for (int s = threadIdx.x; s < bk.S; s += LS_THREADS) {
        int st, slot = -1;
        if (active[s] == 0) {
            st = MYSLAM_LOOP_BANK_IDLE;
        } else if (verify_status[s] == MYSLAM_VERIFY_CONFIRMED) {
            bk.last_closed[s] = (int64_t)cur_id[s];
            st = MYSLAM_LOOP_BANK_CLOSED;
        } else {
            const int n = ls_clamp(bk.n[s], bk.K);
            if (n >= bk.K) st = MYSLAM_ERR_CAPACITY;
            else if (n > 0 && cur_id[s] <= bk.ids[(size_t)s * bk.K + n - 1]) st = MYSLAM_ERR_INVALID;      // std::map order: ids ascend strictly
            else { st = MYSLAM_LOOP_BANK_STORED; slot = n; }
        }
        bk.put_slot[s] = slot;
        add[s] = slot >= 0 ? 1 : 0;
        status[s] = st;
    }
}

// finish, launch b: item s of process_keyframes_batch's outputs -> slot put_slot[s] of stream s
__global__ void __launch_bounds__(LS_THREADS) k_lbank_put(const LbBank bk, const uint64_t* __restrict__ cur_id, const myslam_keypoint* __restrict__ kps,
                                                          const uint8_t* __restrict__ desc, const int32_t* __restrict__ counts,
                                                          const int32_t* __restrict__ kf_status, const int32_t* __restrict__ lm,
                                                          const int32_t* __restrict__ n_feat) {
    const int s = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const int plan = bk.put_slot[s];
    if (plan < 0 || plan >= bk.K) return;
    const LsStore st = lb_stream(bk, s);
    const size_t slot = (size_t)plan;
    const int n = (kf_status && kf_status[s] != 0) ? 0 : ls_clamp(counts[s], st.cap);      // a key-frame the extractor refused is kept, with no rows
    const int nf = ls_clamp(n_feat[s], st.feat_cap);
    if (chunk == 0 && threadIdx.x == 0) {
        st.rows[slot] = n;
        st.nfeat[slot] = nf;
        st.ids[slot] = cur_id[s];
        *st.size = plan + 1;
    }
    ls_copy(st.kps + slot * st.cap_st, kps + (size_t)s * st.cap, (size_t)n * LS_KP_BYTES, chunk, nchunks);
    ls_copy(st.desc + slot * st.cap_st * 32, desc + (size_t)s * st.cap * 32, (size_t)n * 32, chunk, nchunks);
    ls_copy(st.lm + slot * st.feat_st, lm + (size_t)s * st.feat_cap, (size_t)nf * 4, chunk, nchunks);
}

// set_links / clear_links: item s against stream s's ids and nothing else
__global__ void __launch_bounds__(LS_THREADS) k_lbank_links(const LbBank bk, const LsClear c) {
    __shared__ int s_w[LS_THREADS / WAVE];
    const int s = blockIdx.x;
    const LsStore st = lb_stream(bk, s);
    ls_walk_links(st, c, s, ls_clamp(*st.size, bk.K), s_w);
}

__global__ void __launch_bounds__(LS_THREADS) k_lbank_clear(const LbBank bk, const int32_t* __restrict__ reset) {
    const int s = blockIdx.x * LS_THREADS + threadIdx.x;
    if (s < bk.S && reset[s] != 0) { bk.n[s] = 0; bk.last_closed[s] = -1; }
}

}  // namespace myslam_hip

using namespace myslam_hip;

// Nothing here changes after create but the stream: the calls below are launches over fixed pointers.
struct myslam_loop_bank {
    hipStream_t stream = nullptr;
    LbBank b{};
    BufSet mem;
    size_t item_bytes() const { return (size_t)b.cap * (LS_KP_BYTES + 32) + (size_t)b.feat_cap * 4; }
};

static int lbank_sync(const myslam_loop_bank* h) {
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    return MYSLAM_OK;
}

// `n` slots of `width` bytes between a host array of pitch `width` and the stream's slots of pitch `pitch`, complete on return
static int lbank_copy_slots(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, int n, hipMemcpyKind kind) {
    if (n <= 0) return MYSLAM_OK;
    const hipStream_t st = host_call_stream();
    if (!st) return MYSLAM_ERR_HIP;
    MYSLAM_HIP_CHECK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, (size_t)n, kind, st));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    return MYSLAM_OK;
}

static int lbank_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    const hipStream_t st = host_call_stream();
    if (!st) return MYSLAM_ERR_HIP;
    return copy_sync(dst, src, bytes, kind, st);
}

extern "C" {

int myslam_loop_bank_create(myslam_loop_bank** out, int streams, int kfs_per_stream, int cap, int feat_cap) {
    if (!out || streams <= 0 || kfs_per_stream <= 0 || cap <= 0 || feat_cap <= 0) return MYSLAM_ERR_INVALID;
    if (cap > LS_MAX_CAP || feat_cap > LS_MAX_FEAT || streams > LS_MAX_GRID_Y) return MYSLAM_ERR_CAPACITY;
    if (need_device()) return MYSLAM_ERR_HIP;
    std::unique_ptr<myslam_loop_bank> h(new myslam_loop_bank());
    LbBank& b = h->b;
    b.S = streams; b.K = kfs_per_stream; b.cap = cap; b.feat_cap = feat_cap;
    b.cap_st = ls_stride(cap); b.feat_st = ls_stride(feat_cap);
    const size_t S = (size_t)streams, SK = S * (size_t)kfs_per_stream;
    const int oom = MYSLAM_ERR_CAPACITY;
    int rc;
    if ((rc = h->mem.own(b.kps, SK * b.cap_st, oom)) || (rc = h->mem.own(b.desc, SK * b.cap_st * 32, oom)) || (rc = h->mem.own(b.lm, SK * b.feat_st, oom)) ||
        (rc = h->mem.own(b.rows, SK, oom)) || (rc = h->mem.own(b.nfeat, SK, oom)) || (rc = h->mem.own(b.ids, SK, oom)) || (rc = h->mem.own(b.n, S, oom)) ||
        (rc = h->mem.own(b.last_closed, S, oom)) || (rc = h->mem.own(b.put_slot, S, oom)))
        return rc;
    // every stream starts empty with no loop closed; every byte reads the same on every run (never the legacy stream, common.h)
    const hipStream_t us = host_call_stream();
    if (!us) return MYSLAM_ERR_HIP;
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.kps, 0, SK * b.cap_st * LS_KP_BYTES, us));
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.desc, 0, SK * b.cap_st * 32, us));
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.lm, 0, SK * b.feat_st * sizeof(int32_t), us));
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.rows, 0, SK * sizeof(int32_t), us));
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.nfeat, 0, SK * sizeof(int32_t), us));
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.ids, 0, SK * sizeof(uint64_t), us));
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.n, 0, S * sizeof(int32_t), us));
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.last_closed, 0xFF, S * sizeof(int64_t), us));      // -1
    MYSLAM_HIP_CHECK(hipMemsetAsync(b.put_slot, 0xFF, S * sizeof(int32_t), us));         // -1
    MYSLAM_HIP_CHECK(hipStreamSynchronize(us));
    *out = h.release();
    return MYSLAM_OK;
}

int myslam_loop_bank_destroy(myslam_loop_bank* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_loop_bank_set_stream(myslam_loop_bank* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    return MYSLAM_OK;
}

int myslam_loop_bank_view(const myslam_loop_bank* h, myslam_loop_bank_arrays* out) {
    if (!h || !out) return MYSLAM_ERR_INVALID;
    const LbBank& b = h->b;
    *out = myslam_loop_bank_arrays{b.kps, b.desc, b.lm, b.rows, b.nfeat, b.ids, b.n, b.last_closed, b.put_slot,
                                   b.S, b.K, b.cap, b.feat_cap, (int64_t)b.cap_st, (int64_t)b.feat_st};
    return MYSLAM_OK;
}

int myslam_loop_bank_launches_per_finish(void) { return 2; }

int myslam_loop_bank_gate_batch(myslam_loop_bank* h, const int64_t* d_new_kf_id, const int32_t* d_item_status, int status_stride, int32_t* d_active,
                                int32_t* d_status) {
    if (!h || !d_new_kf_id || !d_active || !d_status || (d_item_status && status_stride <= 0)) return MYSLAM_ERR_INVALID;
    hipLaunchKernelGGL(k_lbank_gate, dim3((h->b.S + LS_THREADS - 1) / LS_THREADS), dim3(LS_THREADS), 0, h->stream, h->b, d_new_kf_id, d_item_status,
                       status_stride, d_active, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_loop_bank_detect_batch(myslam_loop_bank* h, const uint64_t* d_best_id, const int32_t* d_best_row, const float* d_max_score, const int32_t* d_cnt,
                                  float thr_high, int max_suspected, uint8_t* d_loop_desc, int32_t* d_n_loop, myslam_keypoint* d_loop_pyr,
                                  int32_t* d_loop_feat_landmark, int32_t* d_loop_slot, int32_t* d_status) {
    if (!h || !d_best_id || !d_best_row || !d_max_score || !d_cnt || !d_loop_desc || !d_n_loop || !d_loop_pyr || !d_loop_feat_landmark || !d_loop_slot ||
        !d_status)
        return MYSLAM_ERR_INVALID;
    hipLaunchKernelGGL(k_lbank_detect, dim3(ls_chunks(h->b.S, h->item_bytes()), h->b.S), dim3(LS_THREADS), 0, h->stream, h->b, d_best_id, d_best_row,
                       d_max_score, d_cnt, thr_high, max_suspected, d_loop_desc, d_n_loop, d_loop_pyr, d_loop_feat_landmark, d_loop_slot, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_loop_bank_finish_batch(myslam_loop_bank* h, const uint64_t* d_cur_kf_id, const int32_t* d_active, const int32_t* d_verify_status,
                                  const myslam_keypoint* d_pyr_kps, const uint8_t* d_desc, const int32_t* d_counts, const int32_t* d_kf_status,
                                  const int32_t* d_feat_landmark, const int32_t* d_n_feat, int32_t* d_add, int32_t* d_status) {
    if (!h || !d_cur_kf_id || !d_active || !d_verify_status || !d_pyr_kps || !d_desc || !d_counts || !d_feat_landmark || !d_n_feat || !d_add || !d_status)
        return MYSLAM_ERR_INVALID;
    hipLaunchKernelGGL(k_lbank_plan, dim3(1), dim3(LS_THREADS), 0, h->stream, h->b, d_cur_kf_id, d_active, d_verify_status, d_add, d_status);
    hipLaunchKernelGGL(k_lbank_put, dim3(ls_chunks(h->b.S, h->item_bytes()), h->b.S), dim3(LS_THREADS), 0, h->stream, h->b, d_cur_kf_id, d_pyr_kps, d_desc,
                       d_counts, d_kf_status, d_feat_landmark, d_n_feat);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_loop_bank_links_batch(myslam_loop_bank* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_value, const int32_t* d_n,
                                     int list_cap, const int64_t* d_pending_kf_id, int32_t* d_pending_feat_landmark, int32_t* d_n_set) {
    if (!h || !d_kf_id || !d_tag || !d_n || list_cap <= 0 || (d_pending_kf_id == nullptr) != (d_pending_feat_landmark == nullptr)) return MYSLAM_ERR_INVALID;
    const LsClear c{d_kf_id, d_tag, d_n, list_cap, d_pending_kf_id, d_pending_feat_landmark, d_n_set, d_value};
    hipLaunchKernelGGL(k_lbank_links, dim3(h->b.S), dim3(LS_THREADS), 0, h->stream, h->b, c);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_loop_bank_clear_batch(myslam_loop_bank* h, const int32_t* d_reset) {
    if (!h || !d_reset) return MYSLAM_ERR_INVALID;
    hipLaunchKernelGGL(k_lbank_clear, dim3((h->b.S + LS_THREADS - 1) / LS_THREADS), dim3(LS_THREADS), 0, h->stream, h->b, d_reset);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_loop_bank_load(myslam_loop_bank* h, int s, const uint64_t* ids, const myslam_keypoint* kps, const uint8_t* desc, const int32_t* rows,
                          const int32_t* feat_landmark, const int32_t* n_feat, int n, int64_t last_closed) {
    if (!h || s < 0 || s >= h->b.S || n < 0 || last_closed < -1 || (n > 0 && (!ids || !kps || !desc || !rows || !feat_landmark || !n_feat)))
        return MYSLAM_ERR_INVALID;
    const LbBank& b = h->b;
    if (n > b.K) return MYSLAM_ERR_CAPACITY;
    for (int i = 0; i < n; i++)
        if ((i > 0 && ids[i] <= ids[i - 1]) || rows[i] < 0 || rows[i] > b.cap || n_feat[i] < 0 || n_feat[i] > b.feat_cap) return MYSLAM_ERR_INVALID;
    int rc;
    if ((rc = lbank_sync(h))) return rc;
    const size_t at = (size_t)s * b.K;
    const int32_t cnt = n;
    const hipMemcpyKind up = hipMemcpyHostToDevice;
    if ((rc = lbank_copy_slots(b.kps + at * b.cap_st, b.cap_st * LS_KP_BYTES, kps, (size_t)b.cap * LS_KP_BYTES, (size_t)b.cap * LS_KP_BYTES, n, up)) ||
        (rc = lbank_copy_slots(b.desc + at * b.cap_st * 32, b.cap_st * 32, desc, (size_t)b.cap * 32, (size_t)b.cap * 32, n, up)) ||
        (rc = lbank_copy_slots(b.lm + at * b.feat_st, b.feat_st * 4, feat_landmark, (size_t)b.feat_cap * 4, (size_t)b.feat_cap * 4, n, up)) ||
        (rc = lbank_copy(b.rows + at, rows, (size_t)n * sizeof(int32_t), up)) || (rc = lbank_copy(b.nfeat + at, n_feat, (size_t)n * sizeof(int32_t), up)) ||
        (rc = lbank_copy(b.ids + at, ids, (size_t)n * sizeof(uint64_t), up)) || (rc = lbank_copy(b.last_closed + s, &last_closed, sizeof(last_closed), up)))
        return rc;
    return lbank_copy(b.n + s, &cnt, sizeof(cnt), up);
}

int myslam_loop_bank_get(myslam_loop_bank* h, int s, uint64_t* ids, myslam_keypoint* kps, uint8_t* desc, int32_t* rows, int32_t* feat_landmark,
                         int32_t* n_feat, int kf_room, int* n, int64_t* last_closed) {
    if (!h || s < 0 || s >= h->b.S || kf_room < 0 || !n || !last_closed) return MYSLAM_ERR_INVALID;
    const LbBank& b = h->b;
    int rc;
    if ((rc = lbank_sync(h))) return rc;
    int32_t cnt = 0;
    const hipMemcpyKind down = hipMemcpyDeviceToHost;
    if ((rc = lbank_copy(&cnt, b.n + s, sizeof(cnt), down)) || (rc = lbank_copy(last_closed, b.last_closed + s, sizeof(int64_t), down))) return rc;
    cnt = std::min(std::max(cnt, 0), b.K);
    *n = cnt;
    if (cnt > kf_room) return MYSLAM_ERR_CAPACITY;
    const size_t at = (size_t)s * b.K;
    if (kps && (rc = lbank_copy_slots(kps, (size_t)b.cap * LS_KP_BYTES, b.kps + at * b.cap_st, b.cap_st * LS_KP_BYTES, (size_t)b.cap * LS_KP_BYTES, cnt, down)))
        return rc;
    if (desc && (rc = lbank_copy_slots(desc, (size_t)b.cap * 32, b.desc + at * b.cap_st * 32, b.cap_st * 32, (size_t)b.cap * 32, cnt, down))) return rc;
    if (feat_landmark &&
        (rc = lbank_copy_slots(feat_landmark, (size_t)b.feat_cap * 4, b.lm + at * b.feat_st, b.feat_st * 4, (size_t)b.feat_cap * 4, cnt, down)))
        return rc;
    if (rows && (rc = lbank_copy(rows, b.rows + at, (size_t)cnt * sizeof(int32_t), down))) return rc;
    if (n_feat && (rc = lbank_copy(n_feat, b.nfeat + at, (size_t)cnt * sizeof(int32_t), down))) return rc;
    if (ids && (rc = lbank_copy(ids, b.ids + at, (size_t)cnt * sizeof(uint64_t), down))) return rc;
    return MYSLAM_OK;
}

int myslam_loop_bank_sizes(myslam_loop_bank* h, int32_t* n) {
    if (!h || !n) return MYSLAM_ERR_INVALID;
    int rc;
    if ((rc = lbank_sync(h))) return rc;
    if ((rc = lbank_copy(n, h->b.n,(size_t)h->b.S * sizeof(int32_t), hipMemcpyDeviceToHost))) return rc;
    for (int s = 0; s < h->b.S; s++) n[s] = std::min(std::max(n[s], 0), h->b.K);
    return MYSLAM_OK;
}

}  // extern "C"
