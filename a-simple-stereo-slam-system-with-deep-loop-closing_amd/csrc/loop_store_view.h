// loop_store_view.h — what the loop key-frame store (loop_store.hip) and the bank of per-stream stores (loop_bank.hip) share: the view of one store,
// the copy that moves an item's arrays, the clamp of a device-side count, the chunking of a call and the walk that sets single landmark links.
// One store is `LsStore`; a stream of the bank is an LsStore whose pointers are offset to the stream and whose `size` is the stream's count.
#pragma once
#include <algorithm>

#include "dev_tables.h"

namespace myslam_hip {

constexpr int LS_THREADS = 256;
constexpr int LS_MAX_CAP = 16384, LS_MAX_FEAT = 65536;        // myslam_loop_match_batch's limits
constexpr int LS_MAX_GRID_Y = 65535;
constexpr size_t LS_MIN_CHUNK_BYTES = (size_t)LS_THREADS * 16;  // a chunk is at least one 16-byte access of every lane
constexpr int LS_TARGET_BLOCKS = 2048;                          // 256 CUs x 8 workgroups: what a bandwidth kernel needs in flight
constexpr int LS_KP_BYTES = 28;
static_assert(sizeof(myslam_keypoint) == LS_KP_BYTES, "cv::KeyPoint layout");

// this workgroup's share of `count` elements of T: element i belongs to chunk (i / LS_THREADS) % nchunks.  A lane with more than three elements
// (few chunks per item: calls of many items) keeps four loads in flight; with the chunking of ls_chunks a lane of a small call has one element
// per array, and what is in flight then is the number of workgroups.
template <class T>
__device__ __forceinline__ void ls_copy_as(T* __restrict__ dst, const T* __restrict__ src, size_t count, int chunk, int nchunks) {
    const size_t step = (size_t)nchunks * LS_THREADS;
    size_t i = (size_t)chunk * LS_THREADS + threadIdx.x;
    for (; i + 3 * step < count; i += 4 * step) {
        const T a = src[i], b = src[i + step], c = src[i + 2 * step], d = src[i + 3 * step];
        dst[i] = a; dst[i + step] = b; dst[i + 2 * step] = c; dst[i + 3 * step] = d;
    }
    for (; i < count; i += step) dst[i] = src[i];
}

// bytes [0, bytes) of one item's array, split over the nchunks workgroups of the item
__device__ __forceinline__ void ls_copy(void* dst, const void* src, size_t bytes, int chunk, int nchunks) {
    const uintptr_t both = (uintptr_t)dst | (uintptr_t)src;
    uint8_t* const d8 = static_cast<uint8_t*>(dst);
    const uint8_t* const s8 = static_cast<const uint8_t*>(src);
    size_t done;
    if ((both & 15) == 0) {
        ls_copy_as(static_cast<uint4*>(dst), static_cast<const uint4*>(src), bytes >> 4, chunk, nchunks);
        done = bytes & ~(size_t)15;
    } else if ((both & 3) == 0) {
        ls_copy_as(static_cast<uint32_t*>(dst), static_cast<const uint32_t*>(src), bytes >> 2, chunk, nchunks);
        done = bytes & ~(size_t)3;
    } else {
        ls_copy_as(d8, s8, bytes, chunk, nchunks);
        done = bytes;
    }
    if (chunk == 0 && done + threadIdx.x < bytes) d8[done + threadIdx.x] = s8[done + threadIdx.x];      // at most 15 bytes
}

__device__ __forceinline__ int ls_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct LsStore {
    myslam_keypoint* kps; uint8_t* desc; int32_t* lm;         // slot s at + s * cap_st (x 32) / + s * feat_st
    int32_t* rows; int32_t* nfeat; uint64_t* ids; int32_t* size;
    int cap, feat_cap; size_t cap_st, feat_st;
};

// slot strides: rounded up to 4 key-points / 4 landmark entries, so every slot starts on a 16-byte boundary
inline size_t ls_stride(int n) { return ((size_t)n + 3) & ~(size_t)3; }

// clear_links / set_links: the lists of one call.  Entry j of item b's list names a feature (key-frame id, feature index) whose mpMapPoint the
// optimiser reset (src/backend.cpp:236-247); its link becomes -1 in the pending table (a key-frame that is not put yet) or in the slot that holds
// the id.  With a value per entry (`value`, nullptr = -1 for all) it is the slot a re-linked feature points at afterwards
// (src/loopclosing.cpp:521-530); an entry whose value is below -1 is ignored.  Two entries that name one feature with different values have no
// order: the re-link's lists name a feature once.
struct LsClear {
    const int64_t* kf_id; const int32_t* tag; const int32_t* n; int list_cap;
    const int64_t* pending_kf_id; int32_t* pending_lm; int32_t* n_cleared;
    const int32_t* value;
};

// The walk of item b's list against the store `st`, by one workgroup of LS_THREADS threads (s_w: LS_THREADS / WAVE ints of LDS).  `held`, the number
// of key-frames `st` holds, is read by the caller.  Two entries that name one feature store the same value.
__device__ __forceinline__ void ls_walk_links(const LsStore& st, const LsClear& c, int b, int held, int* s_w) {
    const int t = threadIdx.x;
    const int n = ls_clamp(c.n[b], c.list_cap);
    const int64_t* const ids = c.kf_id + (size_t)b * c.list_cap;
    const int32_t* const tags = c.tag + (size_t)b * c.list_cap;
    const int32_t* const values = c.value ? c.value + (size_t)b * c.list_cap : nullptr;
    const bool pending = c.pending_kf_id != nullptr;
    const int64_t pend_id = pending ? c.pending_kf_id[b] : -1;
    int cleared = 0;
    for (int base = 0; base < n; base += LS_THREADS) {                      // uniform: every thread meets the block in block_rank
        const int j = base + t;
        bool hit = false;
        if (j < n) {
            const int64_t id = ids[j];
            const int tag = tags[j];
            const int v = values ? values[j] : -1;
            if (id >= 0 && tag >= 0 && v >= -1) {
                if (pending && id == pend_id && tag < st.feat_cap) {
                    c.pending_lm[(size_t)b * st.feat_cap + tag] = v;
                    hit = true;
                } else {
                    // a key-frame that closed a loop, and the five after it, are not held (:671-681)
                    const int slot = lower_row(st.ids, held, (uint64_t)id);
                    if (slot < held && st.ids[slot] == (uint64_t)id && tag < st.nfeat[slot]) {
                        st.lm[(size_t)slot * st.feat_st + tag] = v;
                        hit = true;
                    }
                }
            }
        }
        int tot;
        (void)block_rank<LS_THREADS / WAVE>(hit, s_w, tot);
        cleared += tot;
    }
    if (t == 0 && c.n_cleared) c.n_cleared[b] = cleared;
}

// workgroups per item: enough of them over the whole call to fill the chip, none with less than one full-width access per lane
inline int ls_chunks(int items, size_t item_bytes) {
    const size_t most = std::max<size_t>(1, (item_bytes + LS_MIN_CHUNK_BYTES - 1) / LS_MIN_CHUNK_BYTES);
    const size_t want = (size_t)(LS_TARGET_BLOCKS + items - 1) / items;
    return (int)std::max<size_t>(1, std::min(most, want));
}

}  // namespace myslam_hip
