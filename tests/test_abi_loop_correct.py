"""Loop correction for a batch of maps in the C ABI (include/myslam_hip.h, csrc/loop_correct.hip): the handle, myslam_loop_correct_batch and
myslam_loop_correct_structure are declared with their parameter lists, exported, mirrored by api.LoopCorrector with the header's status values, and
named by the C++ facade.  CPU only."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from test_abi import _declared

NAMES = ["myslam_loop_corrector_create", "myslam_loop_corrector_destroy", "myslam_loop_corrector_set_stream", "myslam_loop_correct_batch",
         "myslam_loop_correct_structure"]
PKG = os.path.join(ROOT, "a-simple-stereo-slam-system-with-deep-loop-closing_amd")


def test_entry_points_declared_with_their_parameter_lists_and_exported(pkg):
    names = _declared()
    assert all(n in names for n in NAMES), [n for n in NAMES if n not in names]
    lib = ctypes.CDLL(pkg.build_library())
    assert all(hasattr(lib, n) for n in NAMES)
    protos = pkg.api.header_prototypes()
    assert protos["myslam_loop_corrector_create"] == ("int", ["ptr"] + ["int"] * 5)          # out, max_batch, kf_cap, edge_cap, active_cap, point_cap
    assert protos["myslam_loop_corrector_destroy"] == ("int", ["ptr"])
    assert protos["myslam_loop_corrector_set_stream"] == ("int", ["ptr", "ptr"])
    # h, poses, n_kf, active, n_active, cur, loop, corrected, verify status, e0, e1, meas, n_edges, points, n_points, first_active, first_kf,
    # batch, correct_threshold, max_iters, chi2, iters, status
    assert protos["myslam_loop_correct_batch"] == ("int", ["ptr"] * 17 + ["int", "double", "int"] + ["ptr"] * 3)
    # n_kf, active, n_active, loop, e0, e1, n_edges, separators, chain length, supported
    assert protos["myslam_loop_correct_structure"] == ("int", ["int", "ptr", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "ptr"])
    # the one-map calls stay as they were
    assert protos["myslam_loop_local_fusion"] == ("int", ["ptr", "int", "int", "ptr", "ptr", "ptr", "int"])
    assert protos["myslam_pose_graph_optimize"] == ("int", ["ptr", "int", "ptr", "ptr", "ptr", "ptr", "int", "int", "ptr", "ptr"])
    assert protos["myslam_correct_map_points"] == ("int", ["ptr", "ptr", "int", "ptr", "ptr", "int"])


def test_api_mirrors_the_handle_and_the_status_values(pkg):
    api = pkg.api
    text = open(os.path.join(ROOT, "include", "myslam_hip.h")).read()
    values = {k: int(v) for k, v in re.findall(r"#define MYSLAM_LOOP_CORRECT_(\w+)\s+(-?\d+)", text)}
    assert values == {"DONE": 0, "NOT_NEEDED": 1, "SKIPPED": 2, "FUSED_ONLY": 3, "MAX_SEPARATORS": values["MAX_SEPARATORS"]} and values["MAX_SEPARATORS"] >= 32
    for k, v in values.items():
        assert getattr(api, "LOOP_CORRECT_" + k) == v
    for m in ("correct_batch", "set_stream"):
        assert callable(getattr(api.LoopCorrector, m))
    assert callable(api.loop_correct_structure)
    m = re.search(r"typedef struct myslam_loop_corrector myslam_loop_corrector;", text)
    assert m and "src/loopclosing.cpp:437-463" in text[m.start() - 8000:m.start()] and "src/loopclosing.cpp:437-463" in text[m.start():]
    for lines in (":328-330", ":284-289", ":470-507", ":537-610", ":612-641"):
        assert lines in text[m.start() - 8000:m.start()], lines


def test_structure_entry_needs_no_device(pkg):
    assert pkg.api.loop_correct_structure(8, [6, 7], 5, [4, 3], [1, 2]) == (1, 3, True)


def test_facade_names_the_class_and_compiles(tmp_path):
    txt = open(os.path.join(PKG, "host", "myslam_hip.hpp")).read()
    assert "class LoopCorrector" in txt and all(n in txt for n in NAMES)
    src = tmp_path / "t.cpp"
    src.write_text('#include "myslam_hip.hpp"\nint main() { return sizeof(myslam::LoopCorrector) > 0 && MYSLAM_LOOP_CORRECT_FUSED_ONLY == 3 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(ROOT, "include"), str(src)])
