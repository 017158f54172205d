"""The multi-stream tracker's entry points of the C ABI (include/myslam_hip.h, csrc/tracker.hip): declared, exported, mirrored by api.py with
the record layout of the header, named by the C++ facade.  CPU only."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from test_abi import _declared

NAMES = ["myslam_tracker_create", "myslam_tracker_destroy", "myslam_tracker_set_stream", "myslam_tracker_set_frame", "myslam_tracker_get_frame",
         "myslam_tracker_step_batch", "myslam_tracker_launches_per_step", "myslam_tracker_debug_last_step"]
PKG = os.path.join(ROOT, "a-simple-stereo-slam-system-with-deep-loop-closing_amd")


def test_tracker_entry_points_declared_and_exported(pkg):
    names = _declared()
    assert all(n in names for n in NAMES), [n for n in NAMES if n not in names]
    lib = ctypes.CDLL(pkg.build_library())
    assert all(hasattr(lib, n) for n in NAMES)
    protos = pkg.api.header_prototypes()
    assert protos["myslam_tracker_step_batch"] == ("int", ["ptr", "ptr", "int", "size_t", "ptr"])
    assert protos["myslam_tracker_create"] == ("int", ["ptr"] + ["int"] * 5 + ["double"] * 4 + ["int"] * 5 + ["float"] * 2)
    assert len(protos["myslam_tracker_set_frame"][1]) == 17 and len(protos["myslam_tracker_get_frame"][1]) == 20


def test_api_mirrors_the_record_and_the_calls(pkg):
    api = pkg.api
    text = open(os.path.join(ROOT, "include", "myslam_hip.h")).read()
    body = re.search(r"typedef struct myslam_tracker_result \{(.*?)\} myslam_tracker_result;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+)(\[7\])?;", body)
    assert [f[1] for f in fields] == list(api.TRACKER_RESULT_DTYPE.names)
    assert api.TRACKER_RESULT_DTYPE.itemsize == sum(56 if f[2] else 4 for f in fields) == 80
    for m in ("set_frame", "get_frame", "step_batch", "debug_last_step", "launches_per_step", "set_stream"):
        assert callable(getattr(api.Tracker, m))
    assert callable(getattr(pkg.chain, "StreamBank"))


def test_facade_names_the_class_and_compiles(tmp_path):
    hpp = os.path.join(PKG, "host", "myslam_hip.hpp")
    txt = open(hpp).read()
    assert "class TrackerBank" in txt and all(n in txt for n in NAMES[:6])
    src = tmp_path / "t.cpp"
    src.write_text('#include "myslam_hip.hpp"\nint main() { return sizeof(myslam::TrackerBank::StreamState) > 0 && sizeof(myslam_tracker_result) == 80 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(ROOT, "include"), str(src)])
