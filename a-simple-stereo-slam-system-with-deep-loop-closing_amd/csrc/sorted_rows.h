// sorted_rows.h — rows of an ascending id column, and a device-side count brought within its cap.  Integer code only, for host and device; it
// includes no HIP header, so tests/cpp/sorted_rows_test.cpp compiles it with g++ alone.  dev_tables.h brings it to the kernels.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MYSLAM_HD __host__ __device__ __forceinline__
#else
#define MYSLAM_HD inline
#endif

namespace myslam_hip {

// The one search of every ascending column: a[0, n) non-decreasing, n < 2^30, a[i] and v compared in their common type.
// lower_row -> first index whose value is not below v; upper_row -> first index whose value is above v.
// On ANY input (a column that is not sorted, as in a table that is still being validated) the loop ends after at most log2(n) + 1 rounds, reads
// only a[0, n), and the result lies in [0, n]: 0 <= lo <= hi <= n holds throughout and hi - lo shrinks every round.  n <= 0 gives 0.
template <bool UPPER, class T, class V>
MYSLAM_HD int bound_row(const T* a, int n, V v) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (UPPER ? a[mid] <= v : a[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}
template <class T, class V>
MYSLAM_HD int lower_row(const T* a, int n, V v) { return bound_row<false>(a, n, v); }
template <class T, class V>
MYSLAM_HD int upper_row(const T* a, int n, V v) { return bound_row<true>(a, n, v); }

// row of id v in a[0, n), -1 if absent; of equal ids (no valid table has any) the first row
template <class T>
MYSLAM_HD int find_row(const T* a, int n, int64_t v) {
    const int i = lower_row(a, n, v);
    return i < n && a[i] == v ? i : -1;
}

// A count that device code wrote, as a loop bound: [0, cap].  For readers that go on with what fits; a kernel that refuses an item whose count is
// out of range (k_map_update, the back end's kernels) tests the raw value instead.
MYSLAM_HD int clamped_count(int n, int cap) { const int lo = n > 0 ? n : 0; return lo < cap ? lo : cap; }
MYSLAM_HD int clamped_count(const int32_t* n, int b, int cap) { return clamped_count(n[b], cap); }

}  // namespace myslam_hip
