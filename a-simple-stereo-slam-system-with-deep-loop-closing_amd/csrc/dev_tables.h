// dev_tables.h — the device-side pieces that the units working on the map's tables share (backend.hip, map_archive.hip, tracker.hip and
// k_loop_pairs of match_tri.hip): ordered positions within a block, the search of an ascending id column and the clamp of a device-side count
// (sorted_rows.h), and the view of the back end's tables.  Integer code only: the units are built with different -ffp-contract settings.
#pragma once
#include <type_traits>

#include "common.h"
#include "sorted_rows.h"

namespace myslam_hip {

// lanes below this one whose bit is set in a ballot mask
__device__ __forceinline__ int lane_prefix(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// The one body of the block scans below, and their contract.  Every thread of a block of nw full waves calls it, in uniform control flow; s_w holds
// one int per wave and belongs to the scans.  The lane with `publish` stores its wave's total, the block meets, every thread sums the nw totals
// (-> the totals of the waves below this one, and `total` of all, block-uniform), the block meets again.  So a scan may follow a scan on the same
// s_w, and the two barriers also separate what a chunk read before the call from what it writes after it: a compaction may write a chunk in place,
// at or below where it stood.  There is no barrier before the store: LDS other than s_w that the caller wrote is not published by the call.
__device__ __forceinline__ int wave_totals_below(bool publish, int wave_total, int* s_w, int nw, int& total) {
    const int wv = threadIdx.x >> 6;
    if (publish) s_w[wv] = wave_total;
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < nw; i++) { const int c = s_w[i]; off += i < wv ? c : 0; tot += c; }
    __syncthreads();
    total = tot;
    return off;
}

// exclusive position of this thread's flag among the block's flags in thread order, and their number.  NW: the block's waves where the block size
// is a compile-time constant (the sum unrolls); without it they are blockDim.x / 64.
__device__ __forceinline__ int block_rank_of(bool f, int* s_w, int nw, int& total) {
    const unsigned long long m = __ballot(f);
    return wave_totals_below((threadIdx.x & 63) == 0, __popcll(m), s_w, nw, total) + lane_prefix(m);
}
template <int NW>
__device__ __forceinline__ int block_rank(bool f, int* s_w, int& total) { return block_rank_of(f, s_w, NW, total); }
__device__ __forceinline__ int block_rank(bool f, int* s_w, int& total) { return block_rank_of(f, s_w, blockDim.x >> 6, total); }

// exclusive block-wide prefix sum of v in thread order, and the sum
template <int NW>
__device__ __forceinline__ int block_exsum(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63;
    int inc = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
    return wave_totals_below(lane == WAVE - 1, inc, s_w, NW, total) + inc - v;
}

// The back end's tables (include/myslam_hip.h, myslam_backend_*): batch arrays strided by the caps; item(b) is the one place that states each stride
// and returns the pointers of map b.  A user that does not read a column passes nullptr for it and never touches that pointer of the item.
// What a user may write: KEY the key-frame ids and their count, POSE the key-frame poses and map-point positions, ROWS everything else.
template <bool W, class T> using BeCol = std::conditional_t<W, T, const T>;
template <bool KEY, bool POSE, bool ROWS>
struct BeTablesT {
    BeCol<KEY, int64_t>* kf_id; BeCol<POSE, double>* kf_pose; BeCol<KEY, int32_t>* n_kf;
    BeCol<ROWS, int64_t>* mp_id; BeCol<POSE, double>* mp_pos; BeCol<ROWS, uint8_t>* mp_outlier; BeCol<ROWS, int32_t>* n_mp;
    BeCol<ROWS, int32_t>* obs_mp; BeCol<ROWS, int32_t>* obs_kf; BeCol<ROWS, uint8_t>* obs_flags; BeCol<ROWS, float>* obs_uv; BeCol<ROWS, int32_t>* obs_tag;
    BeCol<ROWS, int32_t>* n_obs;
    int kf_cap, mp_cap, obs_cap;
    struct Item {
        BeCol<KEY, int64_t>* kf_id; BeCol<POSE, double>* kf_pose; BeCol<ROWS, int64_t>* mp_id; BeCol<POSE, double>* mp_pos; BeCol<ROWS, uint8_t>* mp_outlier;
        BeCol<ROWS, int32_t>* obs_mp; BeCol<ROWS, int32_t>* obs_kf; BeCol<ROWS, uint8_t>* obs_flags; BeCol<ROWS, float>* obs_uv; BeCol<ROWS, int32_t>* obs_tag;
    };
    __device__ __forceinline__ Item item(int b) const {
        const size_t k = (size_t)b * kf_cap, m = (size_t)b * mp_cap, o = (size_t)b * obs_cap;
        return {kf_id + k, kf_pose + k * 7, mp_id + m, mp_pos + m * 3, mp_outlier + m, obs_mp + o, obs_kf + o, obs_flags + o, obs_uv + o * 2, obs_tag + o};
    }
};
using BeTables = BeTablesT<false, true, true>;          // optimise: key-frames neither come nor go
using InsTables = BeTablesT<true, true, true>;          // insert: all in/out
using BeTablesRead = BeTablesT<false, false, false>;    // the archive's update and loop inputs, the tracker's update: read only
using BeTablesPose = BeTablesT<false, true, false>;     // the archive's write-back: poses and positions follow their ids

}  // namespace myslam_hip
