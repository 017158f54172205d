// csrc/sorted_rows.h on the host: lower_row / upper_row / find_row against std::lower_bound / std::upper_bound on every small column, their
// promise on columns that are not sorted, and clamped_count.  Every column is a heap block of exactly n elements, so a read outside a[0, n) is
// AddressSanitizer's to report.  Built with AddressSanitizer + UBSan by tests/test_sorted_rows.py; exit status 0 and "SORTED ROWS OK" = every check held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "sorted_rows.h"

using namespace myslam_hip;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static long g_sorted = 0, g_unsorted = 0;

// every column of length 0..max_n over `alphabet` (ascending, 4 values): the non-decreasing ones against the standard library for every probe,
// the others (up to unsorted_max_n) for the range of the result
template <class T, class V>
static void all_columns(const std::vector<T>& alphabet, const std::vector<V>& probes, int max_n, int unsorted_max_n) {
    const int A = (int)alphabet.size();
    for (int n = 0; n <= max_n; n++) {
        long count = 1;
        for (int i = 0; i < n; i++) count *= A;
        for (long code = 0; code < count; code++) {
            std::vector<T> col(n);
            long c = code;
            for (int i = 0; i < n; i++) { col[i] = alphabet[c % A]; c /= A; }
            const bool sorted = std::is_sorted(col.begin(), col.end());
            if (!sorted && n > unsorted_max_n) continue;
            const T* a = col.data();
            for (const V v : probes) {
                const int lo = lower_row(a, n, v), up = upper_row(a, n, v), f = find_row(a, n, (int64_t)v);
                if (!sorted) {                                  // any input: the loops end, read nothing outside the column, and stay in [0, n]
                    CHECK(lo >= 0 && lo <= n && up >= 0 && up <= n && f >= -1 && f < n);
                    CHECK(f < 0 || a[f] == (T)v);
                    continue;
                }
                const int slo = (int)(std::lower_bound(col.begin(), col.end(), (T)v) - col.begin());
                const int sup = (int)(std::upper_bound(col.begin(), col.end(), (T)v) - col.begin());
                CHECK(lo == slo);
                CHECK(up == sup);
                CHECK(f == (slo < sup ? slo : -1));             // the FIRST row that holds v, -1 when none does
            }
            (sorted ? g_sorted : g_unsorted)++;
        }
    }
}

int main() {
    // the issue's grid: alphabet {-1, 0, 1, 2}, probes -2 .. 3 (absent below, between equal neighbours' runs, and above included)
    const std::vector<int> probes = {-2, -1, 0, 1, 2, 3};
    all_columns<int32_t, int>({-1, 0, 1, 2}, probes, 6, 5);                           // the int32 row columns against an int (obs_mp against a row)
    all_columns<int64_t, int64_t>({-1, 0, 1, 2}, {-2, -1, 0, 1, 2, 3}, 6, 5);         // the id columns
    all_columns<int64_t, int>({-1, 0, 1, 2}, probes, 6, 5);                           // an id column against an int: compared as int64
    // the ends of the id range: no compare wraps
    const int64_t lo = INT64_MIN, hi = INT64_MAX;
    all_columns<int64_t, int64_t>({lo, lo + 1, hi - 1, hi}, {lo, lo + 1, lo + 2, -1, 0, 1, hi - 2, hi - 1, hi}, 6, 5);
    all_columns<int64_t, int64_t>({lo, 0, 1, hi}, {lo, lo + 1, -1, 0, 1, 2, hi - 1, hi}, 6, 5);

    // find_row: absent below, between and above; a duplicated id gives its first row
    {
        const std::vector<int64_t> col = {10, 20, 20, 20, 40};
        const int64_t* a = col.data();
        const int n = (int)col.size();
        CHECK(find_row(a, n, 5) == -1 && find_row(a, n, 30) == -1 && find_row(a, n, 41) == -1);
        CHECK(find_row(a, n, 10) == 0 && find_row(a, n, 20) == 1 && find_row(a, n, 40) == 4);
        CHECK(lower_row(a, n, (int64_t)20) == 1 && upper_row(a, n, (int64_t)20) == 4);
        CHECK(find_row(a, 0, 10) == -1 && lower_row(a, 0, (int64_t)10) == 0 && upper_row(a, 0, (int64_t)10) == 0);
        CHECK(find_row(a, -3, 10) == -1 && lower_row(a, -3, (int64_t)10) == 0);          // a negative count reads nothing
        const std::vector<int32_t> c32 = {7, 7, 7};
        CHECK(find_row(c32.data(), 3, 7) == 0 && find_row(c32.data(), 3, 6) == -1 && find_row(c32.data(), 3, 8) == -1);
        CHECK(find_row(c32.data(), 3, (int64_t)7 + ((int64_t)1 << 32)) == -1);           // an id outside the column's type is absent, not truncated
    }

    // clamped_count: [0, cap], from a value and from a count array
    {
        CHECK(clamped_count(-1, 8) == 0 && clamped_count(INT32_MIN, 8) == 0 && clamped_count(0, 8) == 0 && clamped_count(5, 8) == 5);
        CHECK(clamped_count(8, 8) == 8 && clamped_count(9, 8) == 8 && clamped_count(INT32_MAX, 8) == 8 && clamped_count(3, 0) == 0);
        const std::vector<int32_t> n = {-7, 3, 100};
        CHECK(clamped_count(n.data(), 0, 10) == 0 && clamped_count(n.data(), 1, 10) == 3 && clamped_count(n.data(), 2, 10) == 10);
    }
    CHECK(g_sorted > 0 && g_unsorted > 0);
    printf("SORTED ROWS OK (%ld sorted columns, %ld unsorted)\n", g_sorted, g_unsorted);
    return 0;
}
