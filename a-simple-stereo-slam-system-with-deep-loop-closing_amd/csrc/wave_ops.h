// wave_ops.h — the wave-wide pieces every unit shares, one copy each: the DPP move / add, the DPP wave sum and inclusive scan, the __shfl_xor
// butterfly sum, cv::BORDER_REFLECT_101, and the exact f32 -> 3 x bf16 split.  common.h includes this header, so every unit sees it.
//
// TWO wave sums live here on purpose and are NOT interchangeable:
//   wave_sum_lane63   DPP network, quad -> half row -> row -> row broadcasts; the total is valid in lane 63 only
//   wave_reduce_sum   __shfl_xor butterfly, distances 32, 16, ... 1; every lane receives the total
// They add the 64 values in different orders, so for f32 / f64 their results differ in the last bits; each caller's recorded results depend on
// the one it calls.  The four __shfl_up inclusive scans (ba.hip, orb_kernels.hip x 2, dev_tables.h) are likewise left where they are: moving them to
// wave_incl_scan would change the instructions of hot kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sorted_rows.h"       // MYSLAM_HD

namespace myslam_hip {

// cv::BORDER_REFLECT_101 index of p in [0, len): gfedcb|abcdefgh|gfedcba
MYSLAM_HD int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = (p < 0) ? -p : 2 * len - 2 - p;
    return p;
}

// v of the lane that DPP control CTRL names, in the rows of ROW_MASK; 0 in the other rows and where CTRL names no source lane.
// 64-bit values go as two 32-bit halves.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false); }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float v) { return __int_as_float(dpp_mov<CTRL, ROW_MASK>(__float_as_int(v))); }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_mov(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = dpp_mov<CTRL, ROW_MASK>(lo);
    const int hi2 = dpp_mov<CTRL, ROW_MASK>(hi);
    return __hiloint2double(hi2, lo2);
}
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ T dpp_add(T v) { return v + dpp_mov<CTRL, ROW_MASK>(v); }

// wave sum on the DPP network (no LDS crossbar): the total lands in lane 63
template <typename T>
__device__ __forceinline__ T wave_sum_lane63(T v) {
    v = dpp_add<0xB1, 0xf>(v);      // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xf>(v);      // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xf>(v);     // row_half_mirror
    v = dpp_add<0x140, 0xf>(v);     // row_mirror: every lane holds its 16-lane row sum
    v = dpp_add<0x142, 0xa>(v);     // row_bcast15 into rows 1 and 3
    v = dpp_add<0x143, 0xc>(v);     // row_bcast31 into rows 2 and 3
    return v;
}

// inclusive prefix sum over the 64 lanes on the DPP network (lanes without a source add zero); int, or uint64_t as two halves and one 64-bit add
// per step.  The halves are rejoined in this body and not in a dpp_mov of their own: behind a call the compiler splits every 64-bit add in two.
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
#define MYSLAM_SCAN_STEP(CTRL, ROWS)                                                              \
    if constexpr (sizeof(T) == 8) {                                                               \
        const uint32_t l2 = (uint32_t)dpp_mov<CTRL, ROWS>((int)(uint32_t)v);                      \
        const uint32_t h2 = (uint32_t)dpp_mov<CTRL, ROWS>((int)(uint32_t)(v >> 32));              \
        v += ((uint64_t)h2 << 32) | l2;                                                           \
    } else {                                                                                      \
        v += dpp_mov<CTRL, ROWS>(v);                                                              \
    }
    MYSLAM_SCAN_STEP(0x111, 0xf)    // row_shr:1
    MYSLAM_SCAN_STEP(0x112, 0xf)    // row_shr:2
    MYSLAM_SCAN_STEP(0x114, 0xf)    // row_shr:4
    MYSLAM_SCAN_STEP(0x118, 0xf)    // row_shr:8
    MYSLAM_SCAN_STEP(0x142, 0xa)    // row_bcast15 -> rows 1, 3
    MYSLAM_SCAN_STEP(0x143, 0xc)    // row_bcast31 -> rows 2, 3
#undef MYSLAM_SCAN_STEP
    return v;
}

// butterfly sum: every lane receives the total (see the header comment: not the order of wave_sum_lane63)
template <typename T>
__device__ __forceinline__ T wave_reduce_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a = h + m + l exactly, three bf16 pieces (8 + 8 + 8 significand bits, round-to-nearest conversions, exact residuals); two elements per dword, a0 low
__device__ __forceinline__ void bf16_split3(float a0, float a1, uint32_t& h, uint32_t& m, uint32_t& l) {
    const __bf16 h0 = (__bf16)a0, h1 = (__bf16)a1;
    const float r0 = a0 - (float)h0, r1 = a1 - (float)h1;
    const __bf16 m0 = (__bf16)r0, m1 = (__bf16)r1;
    const float q0 = r0 - (float)m0, q1 = r1 - (float)m1;
    const __bf16 l0 = (__bf16)q0, l1 = (__bf16)q1;
    h = (uint32_t)__builtin_bit_cast(unsigned short, h0) | ((uint32_t)__builtin_bit_cast(unsigned short, h1) << 16);
    m = (uint32_t)__builtin_bit_cast(unsigned short, m0) | ((uint32_t)__builtin_bit_cast(unsigned short, m1) << 16);
    l = (uint32_t)__builtin_bit_cast(unsigned short, l0) | ((uint32_t)__builtin_bit_cast(unsigned short, l1) << 16);
}

}  // namespace myslam_hip
