"""csrc/sorted_rows.h, the one search of every ascending id column (lower_row / upper_row / find_row) and clamped_count, on the host:
tests/cpp/sorted_rows_test.cpp runs them under AddressSanitizer + UBSan against std::lower_bound / std::upper_bound on every non-decreasing column of
length 0 to 6 over four values (int32 and int64 columns, the ends of the int64 range), checks the first row of a duplicated id and -1 for an absent
one, and on every column that is NOT sorted that the loop ends with a result in [0, n] and no read outside the column.  The header includes no HIP
header: g++ alone."""
import os
import subprocess

from conftest import PKG_DIR, ROOT


def test_sorted_rows_against_the_standard_library(tmp_path):
    exe = str(tmp_path / "sorted_rows_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(PKG_DIR, "csrc"), os.path.join(ROOT, "tests", "cpp", "sorted_rows_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "SORTED ROWS OK" in r.stdout, r.stdout + r.stderr[-3000:]
