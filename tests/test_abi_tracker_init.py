"""StereoInit's entry points of the C ABI (include/myslam_hip.h, csrc/tracker.hip): declared, exported, mirrored by api.py and chain.StreamBank,
named by the C++ facade; the header block cites the reference lines its rules come from and stands after the turn's; the turn's ABI is as it
was.  CPU only."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from test_abi import _declared

NAMES = ["myslam_tracker_reset_stream", "myslam_tracker_init_masks", "myslam_tracker_init_batch", "myslam_tracker_init_launches"]
PKG = os.path.join(ROOT, "a-simple-stereo-slam-system-with-deep-loop-closing_amd")


def test_entry_points_declared_and_exported(pkg):
    names = _declared()
    assert all(n in names for n in NAMES), [n for n in NAMES if n not in names]
    lib = ctypes.CDLL(pkg.build_library())
    assert all(hasattr(lib, n) for n in NAMES)
    protos = pkg.api.header_prototypes()
    assert protos["myslam_tracker_reset_stream"] == ("int", ["ptr", "int", "int", "int64_t", "int64_t", "int"])
    assert protos["myslam_tracker_init_masks"] == protos["myslam_tracker_keyframe_masks"] == ("int", ["ptr", "ptr", "int", "size_t"])
    assert protos["myslam_tracker_init_batch"] == ("int", ["ptr", "ptr", "ptr", "int", "size_t", "ptr", "ptr", "int", "double", "int"] + ["ptr"] * 13)
    assert protos["myslam_tracker_init_launches"] == protos["myslam_tracker_keyframe_launches"]
    # the thirteen outputs are the turn's, in its order; what was there stays as it was
    assert protos["myslam_tracker_keyframe_batch"] == ("int", ["ptr", "ptr", "int", "size_t", "ptr", "ptr", "int", "double"] + ["ptr"] * 13)
    text = open(os.path.join(ROOT, "include", "myslam_hip.h")).read()
    outs = lambda name: re.findall(r"\bd_\w+", text[text.index("int " + name + "("):].split(";")[0])[-13:]
    assert outs("myslam_tracker_init_batch") == outs("myslam_tracker_keyframe_batch") and outs("myslam_tracker_init_batch")[0] == "d_new_kf_id"
    assert pkg.api.TRACKER_RESULT_DTYPE.itemsize == 80


def test_header_states_the_rules_with_their_reference_lines():
    text = open(os.path.join(ROOT, "include", "myslam_hip.h")).read()
    start, end = text.index("StereoInit on the device"), text.index("#define MYSLAM_TRACKER_INIT_RETRY")
    assert text.index("#define MYSLAM_TRACKER_NO_TURN") < text.index("int myslam_tracker_set_image_batch(") < start < end, "after the turn's prototypes"
    block = text[start:end]
    for cite in ("282-295", "385-417", "312-313", "427-428", "441-443", "305-309", "319-323", "350-352", "358-361", "285-287", ":291"):
        assert cite in block, cite
    for word in ("ELIGIBLE", "MYSLAM_TRACKER_INIT_RETRY", "MYSLAM_TRACKER_NO_TURN", "MYSLAM_ERR_CAPACITY", "MYSLAM_ERR_INVALID", "EMPTY",
                 "myslam_backend_insert_keyframe_batch", "prev_image = NULL", "3 + 2 x (pyramid levels", "init_good may be any int", "X itself"):
        assert word in block, word
    assert re.search(r"#define MYSLAM_TRACKER_INIT_RETRY\s+2\b", text) and re.search(r"#define MYSLAM_TRACKER_NO_TURN\s+1\b", text)


def test_api_and_chain_mirror_the_calls(pkg):
    api = pkg.api
    for m in ("reset_stream", "init_masks", "init_batch", "init_launches"):
        assert callable(getattr(api.Tracker, m)), m
    assert api.Tracker.INIT_RETRY == 2 and api.Tracker.NO_TURN == 1
    bank = pkg.chain.StreamBank
    assert bank.device_init is False and callable(bank.device_init_turn) and callable(bank.enqueue_init)
    assert "resync" in bank.device_init_turn.__code__.co_varnames


def test_facade_names_the_calls_and_compiles(tmp_path):
    txt = open(os.path.join(PKG, "host", "myslam_hip.hpp")).read()
    assert all(n in txt for n in NAMES), [n for n in NAMES if n not in txt]
    src = tmp_path / "t.cpp"
    src.write_text('#include "myslam_hip.hpp"\n'
                   "int main() { auto a = &myslam::TrackerBank::ResetStream; auto b = &myslam::TrackerBank::InitMasks; auto c = &myslam::TrackerBank::InitBatch;\n"
                   "  auto d = &myslam::TrackerBank::initLaunches; return a && b && c && d && MYSLAM_TRACKER_INIT_RETRY == 2 ? 0 : 1; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(ROOT, "include"), str(src)])
