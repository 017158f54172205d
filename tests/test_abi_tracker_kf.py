"""The key-frame turn's entry points of the C ABI (include/myslam_hip.h, csrc/tracker.hip): declared, exported, mirrored by api.py, named by the
C++ facade; the header cites the reference lines the rules come from; the existing tracker ABI is as it was.  CPU only."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from test_abi import _declared

NAMES = ["myslam_tracker_set_ids", "myslam_tracker_get_ids", "myslam_tracker_keyframe_masks", "myslam_tracker_keyframe_batch",
         "myslam_tracker_keyframe_launches", "myslam_tracker_update_from_map_batch", "myslam_tracker_set_image_batch", "myslam_tracker_debug_last_turn",
         "myslam_tracker_debug_freeze"]
PKG = os.path.join(ROOT, "a-simple-stereo-slam-system-with-deep-loop-closing_amd")


def test_entry_points_declared_and_exported(pkg):
    names = _declared()
    assert all(n in names for n in NAMES), [n for n in NAMES if n not in names]
    lib = ctypes.CDLL(pkg.build_library())
    assert all(hasattr(lib, n) for n in NAMES)
    protos = pkg.api.header_prototypes()
    assert protos["myslam_tracker_set_ids"] == ("int", ["ptr", "int", "ptr", "int", "int64_t", "int64_t", "int64_t"])
    assert protos["myslam_tracker_get_ids"] == ("int", ["ptr", "int"] + ["ptr"] * 6)
    assert protos["myslam_tracker_keyframe_masks"] == ("int", ["ptr", "ptr", "int", "size_t"])
    assert protos["myslam_tracker_keyframe_batch"] == ("int", ["ptr", "ptr", "int", "size_t", "ptr", "ptr", "int", "double"] + ["ptr"] * 13)
    assert protos["myslam_tracker_update_from_map_batch"] == ("int", ["ptr", "ptr", "ptr", "ptr", "int", "ptr", "ptr", "ptr", "ptr", "int"])
    assert protos["myslam_tracker_set_image_batch"] == ("int", ["ptr", "ptr", "int", "size_t", "ptr"])
    # what was there stays as it was
    assert len(protos["myslam_tracker_set_frame"][1]) == 17 and len(protos["myslam_tracker_get_frame"][1]) == 20
    assert pkg.api.TRACKER_RESULT_DTYPE.itemsize == 80


def test_header_states_the_rules_with_their_reference_lines():
    text = open(os.path.join(ROOT, "include", "myslam_hip.h")).read()
    block = text[text.index("Key-frame turns on the device"):text.index("#define MYSLAM_TRACKER_NO_TURN")]
    for cite in ("302-328", "335-379", "451-488", "422-446", "305-309", "319-323", "342-353", "358-361", "456-485", "deeplcd.cpp:46"):
        assert cite in block, cite
    for word in ("ELIGIBLE", "MYSLAM_ERR_CAPACITY", "MYSLAM_ERR_INVALID", "MYSLAM_TRACKER_NO_TURN", "ties to even", "non-finite", "3 + (pyramid levels",
                 "EMPTY key-frame table", "BEFORE the rebuild"):
        assert word in block, word
    assert re.search(r"#define MYSLAM_TRACKER_NO_TURN\s+1\b", text)


def test_api_and_chain_mirror_the_calls(pkg):
    api = pkg.api
    for m in ("set_ids", "get_ids", "keyframe_masks", "keyframe_batch", "update_from_map", "set_image_batch", "keyframe_launches", "debug_last_turn"):
        assert callable(getattr(api.Tracker, m)), m
    assert api.Tracker.NO_TURN == 1 and len(api.Tracker.REPORT_FIELDS) == 8
    assert callable(getattr(pkg.chain.StreamBank, "device_turn"))


def test_facade_names_the_calls_and_compiles(tmp_path):
    txt = open(os.path.join(PKG, "host", "myslam_hip.hpp")).read()
    assert all(n in txt for n in NAMES[:7]), [n for n in NAMES[:7] if n not in txt]
    src = tmp_path / "t.cpp"
    src.write_text('#include "myslam_hip.hpp"\n'
                   "int main() { auto a = &myslam::TrackerBank::SetIds; auto b = &myslam::TrackerBank::KeyframeBatch; auto c = &myslam::TrackerBank::UpdateFromMap;\n"
                   "  auto d = &myslam::TrackerBank::SetImageBatch; auto e = &myslam::TrackerBank::KeyframeMasks; auto f = &myslam::TrackerBank::GetIds;\n"
                   "  auto g = &myslam::TrackerBank::keyframeLaunches; return a && b && c && d && e && f && g ? 0 : 1; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(ROOT, "include"), str(src)])
