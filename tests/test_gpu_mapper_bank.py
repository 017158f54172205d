"""chain.StreamBank with device_map: three rendered streams whose key-frames never leave the device (step -> init / turn -> myslam_mapper_keyframe_batch,
the optimise ON, Map.activeMap.size 3 so that key-frames leave the window and map points come back with prior rows) against the same bank on the host
paths (Chain.grab + hand_off, host_turn, Chain.backend_new_keyframe with the host-pointer BA), loop closing off on both sides.  Per step the result
records are equal byte for byte and so is every feature's resolved view (pixel, landmark id, landmark position, outlier flag: by id, the host's hand_off
compacts the landmark table and the device keeps unreferenced landmarks until the next turn); at the end map_of(s) is the host chain's map.
26 steps, not 22: with KF_EVERY = (4, 4, 5) streams 0 and 1 turn together, so 22 steps hold 7 frames in which some streams make a key-frame and others do
not, and stream 2 makes only two key-frames after its window of 3 is full; 26 steps (which contain the 22) hold 9 such frames and three such key-frames.
Then myslam::Mapper (host/myslam_hip.hpp) in a compiled host program."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_tracker_kf_chain import KF_EVERY, OFFSETS

pytestmark = pytest.mark.gpu

STEPS, WINDOW = 26, 3


def _bank(pkg, api, synth, frames, device):
    chain = pkg.chain
    lcd = api.DeepLCD(synth.calc_weights_handcrafted())
    mk = lambda o: (lambda t: frames[o + t])
    chains = [chain.Chain(chain.HipBackend(api, lcd=lcd), api, synth.SEQ_K, mk(o), cfg={"Map.activeMap.size": WINDOW}, kf_every=k, log=False)
              for o, k in zip(OFFSETS, KF_EVERY)]
    for c in chains:                                     # loop closing off, as tests/test_gpu_tracker_kf_chain.py; the optimise stays ON
        c.lc_insert_new_keyframe = lambda kf: False
    bank = chain.StreamBank(chains, api, cap=1024, landmark_cap=2048)
    bank.device_turns = bank.device_init = bank.device_map = device
    return bank


def resolved(trk, s):
    """every feature of stream s as (pixel bytes, landmark id or -1, position bytes, outlier flag)"""
    st, ids = trk.get_frame(s), trk.get_ids(s)
    out = []
    for (x, y), l in zip(st["xy"], st["lm"]):
        if l < 0:
            out.append((np.float32(x).tobytes() + np.float32(y).tobytes(), -1, b"", 0))
        else:
            out.append((np.float32(x).tobytes() + np.float32(y).tobytes(), int(ids["landmark_id"][l]), np.asarray(st["lm_pos"][l], float).tobytes(),
                        int(st["lm_outlier"][l])))
    return out, st


def test_device_map_equals_the_host_map_step_by_step(api, pkg, synth):
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(max(OFFSETS) + STEPS + 2)]
    dev, host = _bank(pkg, api, synth, frames, True), _bank(pkg, api, synth, frames, False)
    mixed = 0
    for t in range(STEPS):
        a, b = dev.advance(t), host.advance(t)
        assert a == b == [0, 1, 2], (t, a, b, dev.stopped)
        if t:
            assert dev.results().tobytes() == host.results().tobytes(), f"step {t}: result records"
        for s in range(3):
            (fa, sa), (fb, sb) = resolved(dev.trk, s), resolved(host.trk, s)
            assert len(fa) == len(fb), f"step {t} stream {s}: {len(fa)} / {len(fb)} features"
            for i, (x, y) in enumerate(zip(fa, fb)):
                for k, u, v in zip(("pixel", "landmark id", "landmark position", "outlier flag"), x, y):
                    assert u == v, f"step {t} stream {s} feature {i}: {k}"
            for k in ("ref_pose", "last_rel", "rel_motion", "ref_frame_id", "next_frame_id", "status", "frozen"):
                assert np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes(), f"step {t} stream {s}: {k}"
        made = [len(c.kf_frames) for c in dev.chains]
        if t:
            mixed += 0 < sum(m > p for m, p in zip(made, prev)) < 3
        prev = made
    words = [w for _, _, w in dev.map_status]
    print("key-frames per stream", [len(c.kf_frames) for c in dev.chains], "mixed frames", mixed, "mapper calls", len(words))
    assert mixed >= 8, mixed                             # most frames with a key-frame are mixed: some streams turn and others do not
    for s, (cd, ch) in enumerate(zip(dev.chains, host.chains)):
        assert cd.kf_frames == ch.kf_frames and len(cd.kf_frames) - WINDOW >= 3, (s, cd.kf_frames)      # three key-frames at least after the window is full
        assert (cd.status, cd.next_frame_id) == (ch.status, ch.next_frame_id)
        m = dev.map_of(s)
        assert m["kf_id"].tolist() == sorted(ch.all_kfs), s
        for r, k in enumerate(m["kf_id"]):
            assert m["kf_pose"][r].tobytes() == np.asarray(ch.all_kfs[int(k)].pose, float).tobytes(), (s, int(k))
        alive = {int(i): r for r, i in enumerate(m["mp_id"]) if m["mp_state"][r] != 2}
        assert sorted(alive) == sorted(ch.all_mps), (s, len(alive), len(ch.all_mps))
        for i, r in alive.items():
            assert m["mp_pos"][r].tobytes() == np.asarray(ch.all_mps[i].pos, float).tobytes(), (s, i)
        # the trajectory: every frame without a key-frame is the record's pose on both sides; a key-frame's entry is the tracker's estimate here and
        # the pose after that key-frame's optimise in the host chain (Chain.insert_keyframe runs the back end before the pose is noted)
        assert len(cd.poses) == len(ch.poses)
        frame0 = 0
        for f, (p, q) in enumerate(zip(cd.poses, ch.poses)):
            if frame0 + f not in cd.kf_frames:
                assert np.asarray(p).tobytes() == np.asarray(q).tobytes(), (s, f)
        done = [w[s, 5] for w in words if w[s, 0] == 0]
        assert len(done) == len(cd.kf_frames) and done.count(0) >= 2, (s, done)                      # every stream was optimised, not only inserted


def test_cpp_mapper(api, tmp_path):
    """myslam::Mapper (host/myslam_hip.hpp) in a compiled host program: tests/cpp/mapper_test.cpp, two items, one idle"""
    from conftest import PKG_DIR, ROOT
    exe = str(tmp_path / "mapper_test")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "mapper_test.cpp"), "-o", exe,
           "-L" + PKG_DIR, "-lmyslam_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MAPPER TEST OK" in r.stdout, r.stdout + r.stderr
