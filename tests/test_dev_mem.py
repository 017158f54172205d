"""csrc/dev_mem.h, the owner of every device and pinned block of the library, on the host: tests/cpp/dev_mem_test.cpp supplies raw_alloc / raw_free over
malloc (live-block count, "fail the k-th call") and runs under AddressSanitizer + UBSan — a failed growth leaves no size over a freed or null block, a
group's guard stays zero until every member is whole, moves leave nothing behind and nothing leaks.  The header includes no HIP header: g++ alone."""
import os
import subprocess

from conftest import PKG_DIR, ROOT


def test_dev_mem_buf_and_regrow(tmp_path):
    exe = str(tmp_path / "dev_mem_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(PKG_DIR, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "dev_mem_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "DEV MEM OK" in r.stdout, r.stdout + r.stderr[-3000:]
