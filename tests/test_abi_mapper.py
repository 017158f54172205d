"""The mapper in the C ABI (include/myslam_hip.h, MAPPER; csrc/mapper.hip): the entry points are declared with their parameter lists, exported, mirrored
by api.Mapper, chain.StreamBank.device_map / map_of and myslam::Mapper; call-level refusals that need no device; the header's section stands after the
observation archive's users, names its order and what stays out of scope; the entry points it composes keep their prototypes.  CPU only."""
import ctypes
import os
import subprocess

from conftest import ROOT
from test_abi import _declared

NAMES = ["myslam_mapper_create", "myslam_mapper_destroy", "myslam_mapper_set_stream", "myslam_mapper_view", "myslam_mapper_keyframe_batch",
         "myslam_mapper_launches_per_call", "myslam_mapper_reset_item"]
PKG = os.path.join(ROOT, "a-simple-stereo-slam-system-with-deep-loop-closing_amd")


def test_entry_points_declared_with_their_parameter_lists_and_exported(pkg):
    names = _declared()
    assert sorted(n for n in names if n.startswith("myslam_mapper_")) == sorted(NAMES)
    lib = ctypes.CDLL(pkg.build_library())
    assert all(hasattr(lib, n) for n in NAMES)
    protos = pkg.api.header_prototypes()
    assert protos["myslam_mapper_create"] == ("int", ["ptr"] + ["int"] * 10)
    assert protos["myslam_mapper_destroy"] == ("int", ["ptr"]) and protos["myslam_mapper_set_stream"] == ("int", ["ptr", "ptr"])
    assert protos["myslam_mapper_view"] == ("int", ["ptr", "ptr"]) and protos["myslam_mapper_reset_item"] == ("int", ["ptr", "int"])
    assert protos["myslam_mapper_launches_per_call"] == ("int", ["ptr", "int"])
    # h, trk, the thirteen outputs of a turn / an init, window, min_dis_th, fx fy cx cy, huber_delta, chi2_th, max_rounds, iters_per_round, status
    assert protos["myslam_mapper_keyframe_batch"] == ("int", ["ptr"] * 15 + ["int"] + ["double"] * 7 + ["int", "int", "ptr"])
    turn = protos["myslam_tracker_keyframe_batch"][1]
    assert turn[-13:] == ["ptr"] * 13 and protos["myslam_tracker_init_batch"][1][-13:] == ["ptr"] * 13
    # the calls it composes stay as they were
    assert protos["myslam_backend_insert_keyframe_batch"] == ("int", ["ptr"] * 22 + ["int"] + ["ptr"] * 6 + ["int", "ptr", "ptr", "int", "int", "int", "double"] +
                                                              ["ptr"] * 6)
    assert protos["myslam_backend_optimize_batch"] == ("int", ["ptr"] * 14 + ["int"] + ["double"] * 6 + ["int", "int"] + ["ptr"] * 8)
    assert protos["myslam_tracker_update_from_map_batch"] == ("int", ["ptr"] * 4 + ["int"] + ["ptr"] * 4 + ["int"])
    assert protos["myslam_tracker_clear_links_batch"] == ("int", ["ptr"] * 4 + ["int", "ptr"])


def test_the_view_struct_is_the_header_s(pkg):
    """api.MapperTables field for field against typedef struct myslam_mapper_tables"""
    import re
    text = open(os.path.join(ROOT, "include", "myslam_hip.h")).read()
    body = text[text.index("typedef struct myslam_mapper_tables {"):text.index("} myslam_mapper_tables;")]
    body = re.sub(r"/\*.*?\*/", " ", body.split("{", 1)[1], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:
            name = decl.rsplit("*", 1)[1].strip()
            fields.append(("stage_status", 7) if name.startswith("stage_status[") else (name, 1))
        else:
            fields += [(n.strip(), 0) for n in decl.split(None, 1)[1].split(",")]
    got = [(n, (t._length_ if hasattr(t, "_length_") else (1 if t is ctypes.c_void_p else 0))) for n, t in pkg.api.MapperTables._fields_]
    assert got == fields
    assert ctypes.sizeof(pkg.api.MapperTables) == 8 * (sum(max(k, 0) for _, k in fields if k) ) + 4 * sum(1 for _, k in fields if k == 0)
    assert pkg.api.MAPPER_STAGES == ("prior_rows", "insert", "map_after_insert", "obs_after_insert", "optimize", "map_after_optimize", "obs_after_optimize")


def test_call_level_refusals_without_a_handle(pkg):
    api = pkg.api
    lib = api.lib()
    h = ctypes.c_void_p()
    assert lib.myslam_mapper_create(None, 1, 4, 8, 8, 8, 8, 8, 8, 8, 8) == api.ERR_INVALID
    for k in range(10):                                                     # every cap, and the bank size, must be at least 1
        caps = [1, 4, 8, 8, 8, 8, 8, 8, 8, 8]
        caps[k] = 0
        assert lib.myslam_mapper_create(ctypes.byref(h), *caps) == api.ERR_INVALID and not h.value, k
    assert lib.myslam_mapper_create(ctypes.byref(h), 1, 4, 8, 8, 9, 8, 8, 8, 8, 8) == api.ERR_CAPACITY and not h.value      # feat_cap beyond obs_cap
    assert lib.myslam_mapper_create(ctypes.byref(h), 1, 4, 8, 8, 8, 8, 8, 8, 8, 9) == api.ERR_CAPACITY and not h.value      # prior_cap beyond obs_cap
    assert lib.myslam_mapper_destroy(None) == lib.myslam_mapper_set_stream(None, None) == api.ERR_INVALID
    assert lib.myslam_mapper_view(None, None) == lib.myslam_mapper_reset_item(None, 0) == lib.myslam_mapper_launches_per_call(None, 1) == api.ERR_INVALID
    assert lib.myslam_mapper_keyframe_batch(*([None] * 15 + [3, 0.2, 1.0, 1.0, 0.0, 0.0, 5.991, 5.991, 5, 10, None])) == api.ERR_INVALID
    assert (api.MAPPER_IDLE, api.MAPPER_STATUS_WORDS) == (3, 8)


def test_api_chain_header_and_documents_name_the_calls(pkg):
    api, chain = pkg.api, pkg.chain
    for m in ("set_stream", "launches_per_call", "view", "keyframe_batch", "status", "reset_item", "get"):
        assert callable(getattr(api.Mapper, m)), m
    assert chain.StreamBank.device_map is False and callable(chain.StreamBank.map_of)
    text = open(os.path.join(ROOT, "include", "myslam_hip.h")).read()
    i = text.index(" * MAPPER")
    assert i > text.index("int myslam_obs_archive_prior_rows_batch(") and i > text.index("int myslam_tracker_relink_batch(")   # after the archive's users
    section = text[i:text.index("myslam_io_read_png_gray", i)]
    order = ["gate ->", "prior_rows ->", "insert (", "myslam_map_update_batch(AFTER_INSERT)", "myslam_obs_archive_update_batch(AFTER_INSERT)", "optimise (",
             "myslam_map_update_batch(AFTER_OPTIMIZE)", "myslam_obs_archive_update_batch(AFTER_OPTIMIZE", "myslam_tracker_clear_links_batch",
             "myslam_tracker_update_from_map_batch", "-> status"]
    para = section[section.index("Order of one call"):section.index("so both contracts")]
    at = [para.index(s) for s in order]
    assert at == sorted(at), at
    for ref in ("src/backend.cpp:82-121", "BackendRun, :30-37", ":126-266", "src/map.cpp:17-48", "src/loopclosing.cpp:671-681", "src/deeplcd.cpp:46", "OUT OF SCOPE",
                "STICKY", "MYSLAM_MAPPER_IDLE", "MYSLAM_TRACKER_NO_TURN", "MYSLAM_TRACKER_INIT_RETRY", "myslam_graph_begin", "ONE CALL CONSUMES ONE OUTPUT SET",
                "myslam_mapper_reset_item", "myslam_tracker_reset_stream"):
        assert ref in section, ref
    trk = text[text.index("WOULD BE APPENDED"):text.index("myslam_tracker_update_from_map_batch — 1 launch")]
    assert "must take such items out itself" in trk and "myslam_mapper_keyframe_batch" in trk                # the behaviour stays, the pointer is new
    assert "#define MYSLAM_MAPPER_IDLE 3" in text and "#define MYSLAM_MAPPER_STATUS_WORDS 8" in text
    build = open(os.path.join(PKG, "build.py")).read()
    assert '"mapper.hip": []' in build
    launch = open(os.path.join(PKG, "csrc", "backend_launch.h")).read()
    assert "backend_insert_launch" in launch and "backend_optimize_launch" in launch and "d_gate" in launch
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "myslam_mapper_keyframe_batch" in doc and "Backend::BackendRun" in doc
    assert "3.16f" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("README.md", "DESIGN.md"):
        assert "myslam_mapper" in open(os.path.join(ROOT, name)).read(), name


def test_facade_names_the_calls_and_compiles(tmp_path):
    txt = open(os.path.join(PKG, "host", "myslam_hip.hpp")).read()
    assert "class Mapper" in txt and all(n in txt for n in NAMES)
    src = tmp_path / "t.cpp"
    src.write_text('#include "myslam_hip.hpp"\nint main() {\n'
                   '    return (&myslam::Mapper::KeyFrameBatch != nullptr && &myslam::Mapper::ResetItem != nullptr && &myslam::Mapper::View != nullptr &&\n'
                   '            &myslam::Mapper::Status != nullptr && &myslam::Mapper::launchesPerCall != nullptr && &myslam::TrackerBank::handle != nullptr) ? 0 : 1;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-address", "-I" + os.path.join(PKG, "host"),
                           "-I" + os.path.join(ROOT, "include"), str(src)])
