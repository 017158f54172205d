// loop_store.hip — the step between LoopClosing::DetectLoop's scan and MatchFeatures (src/loopclosing.cpp:147, :151) on gfx950: a device-resident store of
// what ProcessNewKF leaves in a KeyFrame (keyframe.h: mvPyramidKeyPoints, mORBDescriptors, and per feature of mvpFeaturesLeft whether mpMapPoint.lock()
// still names a landmark), and one launch that applies `maxScore < thr_high || cnt > 3` to myslam_lcddb_query_batch's outputs and writes the chosen
// key-frames' arrays where myslam_loop_match_batch reads them.
//
// The store is kf_capacity slots of fixed size; slot s holds the s-th key-frame put, ids ascend with the slot.  Nothing ever moves, so a recorded
// launch stays valid; ids, row counts, feature counts and the number of key-frames held are read ON THE DEVICE, so a replay sees what was put after
// the recording.  Slot strides are rounded up to 4 key-points / 4 landmark entries: every slot starts on a 16-byte boundary.
//
// k_loop_store_clear_links (one workgroup per item) sets single entries of stored landmark tables to -1: the features the optimiser reset; with
// a value column (set_links) to the slot a re-linked feature points at.
// The other kernels are copies and nothing else: a 2-D grid (chunk x item), every workgroup repeats its item's decision (two compares and a binary search
// over the ids, all wave-uniform) and then moves its share of the item's three arrays, 16 bytes per lane where source and destination of the item are
// 16-byte aligned (a key-point is 28 bytes: item b of a caller's table starts aligned only when b * cap is a multiple of 4), a dword per lane
// otherwise, bytes for a pointer that is not even 4-byte aligned.  Chunk 0 writes the item's status, slot and counts.
// The view of the store, the copy, the clamp, the chunking and the walk of clear_links live in loop_store_view.h: loop_bank.hip uses them too.
#include "loop_store_view.h"

namespace myslam_hip {

// put: item b of process_keyframes_batch's outputs -> slot first_slot + b.  The ids were copied ahead on the same stream.
__global__ void __launch_bounds__(LS_THREADS) k_loop_store_put(const LsStore st, int first_slot, int new_size, const myslam_keypoint* __restrict__ kps,
                                                               const uint8_t* __restrict__ desc, const int32_t* __restrict__ counts,
                                                               const int32_t* __restrict__ kf_status, const int32_t* __restrict__ lm,
                                                               const int32_t* __restrict__ n_feat) {
    const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const size_t slot = (size_t)first_slot + b;
    const int n = (kf_status && kf_status[b] != 0) ? 0 : ls_clamp(counts[b], st.cap);      // a key-frame the extractor refused is kept, with no rows
    const int nf = ls_clamp(n_feat[b], st.feat_cap);
    if (chunk == 0 && threadIdx.x == 0) {
        st.rows[slot] = n;
        st.nfeat[slot] = nf;
        if (b == 0 && new_size >= 0) *st.size = new_size;
    }
    ls_copy(st.kps + slot * st.cap_st, kps + (size_t)b * st.cap, (size_t)n * LS_KP_BYTES, chunk, nchunks);
    ls_copy(st.desc + slot * st.cap_st * 32, desc + (size_t)b * st.cap * 32, (size_t)n * 32, chunk, nchunks);
    ls_copy(st.lm + slot * st.feat_st, lm + (size_t)b * st.feat_cap, (size_t)nf * 4, chunk, nchunks);
}

// set_landmarks: item b's table and count -> slot slots[b]
__global__ void __launch_bounds__(LS_THREADS) k_loop_store_set_landmarks(const LsStore st, const int32_t* __restrict__ slots, const int32_t* __restrict__ lm,
                                                                         const int32_t* __restrict__ n_feat) {
    const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const size_t slot = (size_t)slots[b];
    const int nf = ls_clamp(n_feat[b], st.feat_cap);
    if (chunk == 0 && threadIdx.x == 0) st.nfeat[slot] = nf;
    ls_copy(st.lm + slot * st.feat_st, lm + (size_t)b * st.feat_cap, (size_t)nf * 4, chunk, nchunks);
}

// detect: the decision of loopclosing.cpp:147 and `_mpLoopKF = _mvDatabase.at(bestId)` (:151) per item, then the gather
__global__ void __launch_bounds__(LS_THREADS) k_loop_detect(const LsStore st, const uint64_t* __restrict__ best_id, const float* __restrict__ max_score,
                                                            const int32_t* __restrict__ cnt, float thr_high, int max_suspected,
                                                            uint8_t* __restrict__ loop_desc, int32_t* __restrict__ n_loop, myslam_keypoint* __restrict__ loop_pyr,
                                                            int32_t* __restrict__ loop_lm, int32_t* __restrict__ loop_slot, int32_t* __restrict__ status) {
    const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const bool lead = chunk == 0 && threadIdx.x == 0;
    // the reference's expression as written: a NaN score is not "less" and goes on to the lookup
    if (max_score[b] < thr_high || cnt[b] > max_suspected) {
        if (lead) { status[b] = MYSLAM_LOOP_DETECT_NO_LOOP; n_loop[b] = 0; loop_slot[b] = -1; }
        return;
    }
    const uint64_t id = best_id[b];
    const int held = *st.size;
    int lo = 0, hi = held;                                      // -> the first slot whose id is not below `id`
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (st.ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    if (lo >= held || st.ids[lo] != id) {
        if (lead) { status[b] = MYSLAM_ERR_INVALID; n_loop[b] = 0; loop_slot[b] = -1; }
        return;
    }
    const size_t slot = (size_t)lo;
    const int n = st.rows[slot], nf = st.nfeat[slot];           // clamped when they were stored
    if (lead) { status[b] = MYSLAM_LOOP_DETECT_CANDIDATE; n_loop[b] = n; loop_slot[b] = lo; }
    ls_copy(loop_pyr + (size_t)b * st.cap, st.kps + slot * st.cap_st, (size_t)n * LS_KP_BYTES, chunk, nchunks);
    ls_copy(loop_desc + (size_t)b * st.cap * 32, st.desc + slot * st.cap_st * 32, (size_t)n * 32, chunk, nchunks);
    ls_copy(loop_lm + (size_t)b * st.feat_cap, st.lm + slot * st.feat_st, (size_t)nf * 4, chunk, nchunks);
}

// clear_links: one workgroup per item.  Entry j of item b's list names a feature (key-frame id, feature index) whose mpMapPoint the optimiser
// reset (src/backend.cpp:236-247); its link becomes -1 in the pending table (a key-frame that is not put yet) or in the slot that holds the id.
// The number of key-frames held is read here, as k_loop_detect reads it.  Two entries that name one feature store the same -1.
// set_links is the same walk with a value per entry (`value`, nullptr = -1 for all): the slot a re-linked feature points at afterwards
// (src/loopclosing.cpp:521-530); an entry whose value is below -1 is ignored.  Two entries that name one feature with different values have no
// order: the re-link's lists name a feature once.  (LsClear and the walk itself: ls_walk_links, loop_store_view.h.)
__global__ void __launch_bounds__(LS_THREADS) k_loop_store_clear_links(const LsStore st, const LsClear c) {
    __shared__ int s_w[LS_THREADS / WAVE];
    ls_walk_links(st, c, blockIdx.x, *st.size, s_w);
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_loop_store {
    int kf_capacity = 0, cap = 0, feat_cap = 0, n = 0;
    hipStream_t stream = nullptr;
    Buf<myslam_keypoint> d_kps; Buf<uint8_t> d_desc; Buf<int32_t> d_lm, d_rows, d_nfeat, d_size, d_slots;
    Buf<uint64_t> d_ids;
    // the ids as the device copies them: slot s is written once, when key-frame s is put, and never again — no copy ever reads a slot that changes
    PinBuf<uint64_t> h_ids;
    // slot lists of set_landmarks_batch on their way to the device: a ring, each part with the event behind its copy
    static constexpr int RING = 4;
    PinBuf<int32_t> h_slots; hipEvent_t slotEv[RING] = {}; bool slotPending[RING] = {}; int ring = 0;
    mutable std::mutex mu;                    // host state: n, stream, the ring
    LsStore view{};

    ~myslam_loop_store() { for (hipEvent_t e : slotEv) if (e) (void)hipEventDestroy(e); }
    size_t item_bytes() const { return (size_t)cap * (LS_KP_BYTES + 32) + (size_t)feat_cap * 4; }
    int find(uint64_t id) const {
        const uint64_t* const b = h_ids.get(), * const e = b + n;
        const uint64_t* it = std::lower_bound(b, e, id);
        return (it != e && *it == id) ? (int)(it - b) : -1;
    }
};

extern "C" {

int myslam_loop_store_create(myslam_loop_store** out, int kf_capacity, int cap, int feat_cap) {
    if (!out || kf_capacity <= 0 || cap <= 0 || feat_cap <= 0) return MYSLAM_ERR_INVALID;
    if (cap > LS_MAX_CAP || feat_cap > LS_MAX_FEAT) return MYSLAM_ERR_CAPACITY;
    if (need_device()) return MYSLAM_ERR_HIP;
    std::unique_ptr<myslam_loop_store> h(new myslam_loop_store());
    h->kf_capacity = kf_capacity; h->cap = cap; h->feat_cap = feat_cap;
    const size_t K = (size_t)kf_capacity, cap_st = ls_stride(cap), feat_st = ls_stride(feat_cap);
    const int oom = MYSLAM_ERR_CAPACITY;
    int rc;
    if ((rc = h->d_kps.renew(K * cap_st, oom)) || (rc = h->d_desc.renew(K * cap_st * 32, oom)) || (rc = h->d_lm.renew(K * feat_st, oom)) ||
        (rc = h->d_rows.renew(K, oom)) || (rc = h->d_nfeat.renew(K, oom)) || (rc = h->d_ids.renew(K, oom)) || (rc = h->d_slots.renew(K, oom)) ||
        (rc = h->d_size.renew(1, oom)) || (rc = h->h_ids.renew(K, oom)) || (rc = h->h_slots.renew(K * myslam_loop_store::RING, oom)))
        return rc;
    for (auto& e : h->slotEv) MYSLAM_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int32_t zero = 0;
    if ((rc = upload_table(h->d_size, &zero, sizeof(zero)))) return rc;      // complete on return: the first launch may come on any stream
    h->view = LsStore{h->d_kps, h->d_desc, h->d_lm, h->d_rows, h->d_nfeat, h->d_ids, h->d_size, cap, feat_cap, cap_st, feat_st};
    *out = h.release();
    return MYSLAM_OK;
}

int myslam_loop_store_destroy(myslam_loop_store* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_loop_store_set_stream(myslam_loop_store* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->stream = (hipStream_t)hip_stream;
    return MYSLAM_OK;
}

int myslam_loop_store_size(const myslam_loop_store* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->n;
}

int myslam_loop_store_capacity(const myslam_loop_store* h) { return h ? h->kf_capacity : MYSLAM_ERR_INVALID; }

int myslam_loop_store_put_batch(myslam_loop_store* h, const uint64_t* ids, int batch, const myslam_keypoint* d_pyr_kps, const uint8_t* d_desc,
                                const int32_t* d_counts, const int32_t* d_kf_status, const int32_t* d_feat_landmark, const int32_t* d_n_feat) {
    if (!h || !ids || batch <= 0 || !d_pyr_kps || !d_desc || !d_counts || !d_feat_landmark || !d_n_feat) return MYSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < batch; i++)            // std::map order: strictly ascending, behind every id held
        if (i == 0 ? h->n > 0 && ids[0] <= h->h_ids[h->n - 1] : ids[i] <= ids[i - 1]) return MYSLAM_ERR_INVALID;
    if ((long long)h->n + batch > h->kf_capacity) return MYSLAM_ERR_CAPACITY;
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;              // a put is host bookkeeping too: it cannot be replayed
    memcpy(h->h_ids + h->n, ids, sizeof(uint64_t) * (size_t)batch);
    MYSLAM_HIP_CHECK(hipMemcpyAsync(h->d_ids + h->n, h->h_ids + h->n, sizeof(uint64_t) * (size_t)batch, hipMemcpyHostToDevice, h->stream));
    const int chunks = ls_chunks(batch, h->item_bytes());
    for (int b0 = 0; b0 < batch; b0 += LS_MAX_GRID_Y) {
        const int nb = std::min(batch - b0, LS_MAX_GRID_Y);
        // the number of key-frames held changes with the LAST launch: a detect that follows on the stream sees the rows before it sees the count
        const int new_size = b0 + nb == batch ? h->n + batch : -1;
        hipLaunchKernelGGL(k_loop_store_put, dim3(chunks, nb), dim3(LS_THREADS), 0, h->stream, h->view, h->n + b0, new_size,
                           d_pyr_kps + (size_t)b0 * h->cap, d_desc + (size_t)b0 * h->cap * 32, d_counts + b0, d_kf_status ? d_kf_status + b0 : nullptr,
                           d_feat_landmark + (size_t)b0 * h->feat_cap, d_n_feat + b0);
        MYSLAM_HIP_CHECK(hipGetLastError());
    }
    h->n += batch;
    return MYSLAM_OK;
}

int myslam_loop_store_set_landmarks_batch(myslam_loop_store* h, const uint64_t* ids, int n, const int32_t* d_feat_landmark, const int32_t* d_n_feat) {
    if (!h || !ids || n <= 0 || !d_feat_landmark || !d_n_feat) return MYSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (n > h->n) return MYSLAM_ERR_INVALID;                                  // more items than key-frames held: one of them is unknown or repeated
    std::vector<int32_t> slots((size_t)n);
    for (int i = 0; i < n; i++)
        if ((slots[i] = h->find(ids[i])) < 0) return MYSLAM_ERR_INVALID;
    {   // two items for one key-frame would race
        std::vector<int32_t> s(slots);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) return MYSLAM_ERR_INVALID;
    }
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;
    const int r = h->ring; h->ring = (h->ring + 1) % myslam_loop_store::RING;
    if (h->slotPending[r]) MYSLAM_HIP_CHECK(hipEventSynchronize(h->slotEv[r]));  // the copy of four calls ago: long done
    int32_t* const stage = h->h_slots + (size_t)r * h->kf_capacity;
    memcpy(stage, slots.data(), sizeof(int32_t) * (size_t)n);
    MYSLAM_HIP_CHECK(hipMemcpyAsync(h->d_slots, stage, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    MYSLAM_HIP_CHECK(hipEventRecord(h->slotEv[r], h->stream)); h->slotPending[r] = true;
    const int chunks = ls_chunks(n, (size_t)h->feat_cap * 4);
    for (int b0 = 0; b0 < n; b0 += LS_MAX_GRID_Y) {
        const int nb = std::min(n - b0, LS_MAX_GRID_Y);
        hipLaunchKernelGGL(k_loop_store_set_landmarks, dim3(chunks, nb), dim3(LS_THREADS), 0, h->stream, h->view, h->d_slots + b0,
                           d_feat_landmark + (size_t)b0 * h->feat_cap, d_n_feat + b0);
        MYSLAM_HIP_CHECK(hipGetLastError());
    }
    return MYSLAM_OK;
}

int myslam_loop_store_clear_links_batch(myslam_loop_store* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_n, int list_cap, int batch,
                                        const int64_t* d_pending_kf_id, int32_t* d_pending_feat_landmark, int32_t* d_n_cleared) {
    if (!h || !d_kf_id || !d_tag || !d_n || list_cap <= 0 || batch <= 0 || (d_pending_kf_id == nullptr) != (d_pending_feat_landmark == nullptr))
        return MYSLAM_ERR_INVALID;
    if (batch > LS_MAX_GRID_Y) return MYSLAM_ERR_CAPACITY;
    std::lock_guard<std::mutex> lk(h->mu);
    // no host bookkeeping: the ids and their number are read on the device, so the launch may be recorded
    const LsClear c{d_kf_id, d_tag, d_n, list_cap, d_pending_kf_id, d_pending_feat_landmark, d_n_cleared, nullptr};
    hipLaunchKernelGGL(k_loop_store_clear_links, dim3(batch), dim3(LS_THREADS), 0, h->stream, h->view, c);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_loop_store_set_links_batch(myslam_loop_store* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_slot, const int32_t* d_n,
                                      int list_cap, int batch, const int64_t* d_pending_kf_id, int32_t* d_pending_feat_landmark, int32_t* d_n_set) {
    if (!h || !d_kf_id || !d_tag || !d_slot || !d_n || list_cap <= 0 || batch <= 0 || (d_pending_kf_id == nullptr) != (d_pending_feat_landmark == nullptr))
        return MYSLAM_ERR_INVALID;
    if (batch > LS_MAX_GRID_Y) return MYSLAM_ERR_CAPACITY;
    std::lock_guard<std::mutex> lk(h->mu);
    const LsClear c{d_kf_id, d_tag, d_n, list_cap, d_pending_kf_id, d_pending_feat_landmark, d_n_set, d_slot};
    hipLaunchKernelGGL(k_loop_store_clear_links, dim3(batch), dim3(LS_THREADS), 0, h->stream, h->view, c);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_loop_detect_batch(myslam_loop_store* h, const uint64_t* d_best_id, const float* d_max_score, const int32_t* d_cnt, int nq, float thr_high,
                             int max_suspected, uint8_t* d_loop_desc, int32_t* d_n_loop, myslam_keypoint* d_loop_pyr, int32_t* d_loop_feat_landmark,
                             int32_t* d_loop_slot, int32_t* d_status) {
    if (!h || !d_best_id || !d_max_score || !d_cnt || nq <= 0 || !d_loop_desc || !d_n_loop || !d_loop_pyr || !d_loop_feat_landmark || !d_loop_slot ||
        !d_status)
        return MYSLAM_ERR_INVALID;
    if (nq > LS_MAX_GRID_Y) return MYSLAM_ERR_CAPACITY;
    std::lock_guard<std::mutex> lk(h->mu);
    hipLaunchKernelGGL(k_loop_detect, dim3(ls_chunks(nq, h->item_bytes()), nq), dim3(LS_THREADS), 0, h->stream, h->view, d_best_id, d_max_score, d_cnt,
                       thr_high, max_suspected, d_loop_desc, d_n_loop, d_loop_pyr, d_loop_feat_landmark, d_loop_slot, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

}  // extern "C"
