// resize_tab.h — plan-time coordinate tables of k_resize_strip (orb_kernels.hip K1b).  Host only, plain C++ (the table test compiles it alone).
//
// Everything the strip kernel needs before its first load is fixed by the plan's geometry (source and destination size of a level), so the
// host works it out once where the plan is made instead of every wave of every launch: per group of four destination columns one 32-byte
// record, per destination row one 16-byte record.  The values are bit for bit what resize_coord (orb_kernels.hip) yields on the device:
// the same operations in the same order, no contraction, round-to-nearest-even conversions.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace myslam_hip {

// [0] byte offset of sx[0] in a source row (its dword-aligned part | its byte shift in the low two bits)
// [1..3] v_perm selectors of the byte pairs (sx[k], sx[k] + 1) of columns 1..3 in the 8-byte window at sx[0] (column 0's is the constant 0x0c010c00)
// [4..7] the four weight pairs a0 | a1 << 16 (11 bit)
struct ResizeColRec { uint32_t sx0, sel[3], aw[4]; };
// clamped upper source row, 1 = both taps fall on it (the lower one is clamped to it at an image border), b0 << 12, b1 << 12
struct ResizeRowRec { uint32_t srow, same, b0, b1; };
static_assert(sizeof(ResizeColRec) == 32 && sizeof(ResizeRowRec) == 16, "the kernel loads the records as 2 x 16 and 1 x 16 bytes");
constexpr int RESIZE_ROW_SPARE = 2;      // records past the last row (copies of it): the walk keeps the next row's record in flight

// resize_coord of orb_kernels.hip on the host, line by line
#if defined(__clang__)
#define MYSLAM_NO_CONTRACT _Pragma("clang fp contract(off)")
#define MYSLAM_NO_CONTRACT_ATTR
#else
#define MYSLAM_NO_CONTRACT
#define MYSLAM_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#endif
MYSLAM_NO_CONTRACT_ATTR inline void resize_coord_host(int d, double scale, int ssize, bool is_x, int& s, int& c0, int& c1) {
    MYSLAM_NO_CONTRACT
    const double m = ((double)d + 0.5) * scale;          // __dmul_rn((double)d + 0.5, scale)
    const double e = m - 0.5;                            // __dsub_rn(.., 0.5)
    float f = (float)e;                                  // (float): f64 -> f32, round to nearest even
    int si = (int)floorf(f);                             // (int)floorf(f)
    f = f - (float)si;                                   // __fsub_rn(f, (float)si)
    if (is_x) {
        if (si < 0) { f = 0.f; si = 0; }
        if (si >= ssize - 1) { f = 0.f; si = ssize - 1; }
    }
    s = si;
    const float w0 = (1.f - f) * 2048.f, w1 = f * 2048.f;    // __fmul_rn(__fsub_rn(1.f, f), 2048.f), __fmul_rn(f, 2048.f)
    c0 = (int)nearbyintf(w0);                            // __float2int_rn: nearest even (the default rounding mode; both products are exact integers or halves far below 2^31)
    c1 = (int)nearbyintf(w1);
}

// column records of one level: ngroups >= ceil(dw / 4) records (the launcher rounds up to whole strips of 64 groups; groups past the last
// column repeat it, as min(dx4 + k, dw - 1) did in the kernel)
inline void resize_col_records(int sw, int dw, double scale_x, int ngroups, std::vector<ResizeColRec>& out) {
    out.resize((size_t)ngroups);
    for (int g = 0; g < ngroups; g++) {
        int sx[4], a0, a1;
        ResizeColRec& r = out[(size_t)g];
        for (int k = 0; k < 4; k++) {
            resize_coord_host(std::min(4 * g + k, dw - 1), scale_x, sw, true, sx[k], a0, a1);
            r.aw[k] = (uint32_t)a0 | ((uint32_t)a1 << 16);                                   // aw[k] = c0 | c1 << 16
            const uint32_t o = (uint32_t)(sx[k] - sx[0]);                                    // selk[k] = 0x0c000c00 | (o + 1) << 16 | o
            if (k > 0) r.sel[k - 1] = 0x0c000c00u | ((o + 1u) << 16) | o;
        }
        r.sx0 = (uint32_t)sx[0];                                                             // xal = sx[0] & ~3, shift = sx[0] & 3
    }
}

// row records of one level: dh + RESIZE_ROW_SPARE records
inline void resize_row_records(int sh, int dh, double scale_y, std::vector<ResizeRowRec>& out) {
    out.resize((size_t)dh + RESIZE_ROW_SPARE);
    for (int d = 0; d < dh; d++) {
        int sy, b0, b1;
        resize_coord_host(d, scale_y, sh, false, sy, b0, b1);
        const int r0 = std::min(std::max(sy, 0), sh - 1), r1 = std::min(std::max(sy + 1, 0), sh - 1);      // min(max(sy, 0), a.sh - 1), min(max(sy + 1, 0), a.sh - 1)
        out[(size_t)d] = ResizeRowRec{(uint32_t)r0, r0 == r1 ? 1u : 0u, (uint32_t)b0 << 12, (uint32_t)b1 << 12};
    }
    for (int d = dh; d < dh + RESIZE_ROW_SPARE; d++) out[(size_t)d] = out[(size_t)dh - 1];
}

}  // namespace myslam_hip
