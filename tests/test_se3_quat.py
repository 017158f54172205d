"""csrc/se3_quat.h, the SE3 functions myslam_loop_local_fusion shares with the pose-graph kernels, on the host: tests/cpp/se3_quat_test.cpp runs them
under AddressSanitizer + UBSan on the inputs of test_loop_local_fusion (tests/test_gpu_pgo.py: the last seven poses of synth.pose_graph(40, 1, seed=9)
and the corrected current pose).  The fused poses are held to oracle.loop_local_fusion at the bar of that test, atol 1e-12; pg_inv(pg_inv(T)) and
pg_store(pg_load(p)) are checked bit for bit inside the program.  The header includes no HIP header: g++ alone."""
import os
import subprocess

import numpy as np

from conftest import PKG_DIR, ROOT


def test_host_se3_fuses_the_active_poses_as_the_oracle_does(tmp_path, oracle, synth):
    exe = str(tmp_path / "se3_quat_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(PKG_DIR, "csrc"), os.path.join(ROOT, "tests", "cpp", "se3_quat_test.cpp"), "-o", exe])
    poses = synth.pose_graph(40, 1, seed=9)[0][-7:].copy()
    corrected = oracle.se3_compose(poses[6], oracle.se3_exp(np.array([0.3, -0.1, 0.2, 0.02, -0.01, 0.03])))
    fin, fout = str(tmp_path / "in.f64"), str(tmp_path / "out.f64")
    np.concatenate([[7.0, 6.0], poses.ravel(), corrected]).astype(np.float64).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "SE3 QUAT OK (7 poses)" in r.stdout, r.stdout + r.stderr[-3000:]
    got = np.fromfile(fout, np.float64).reshape(7, 7)
    ref, _ = oracle.loop_local_fusion(poses, 6, corrected, np.zeros(0, np.int32), np.zeros((0, 3)))
    assert np.allclose(got, ref, rtol=0, atol=1e-12)
    assert np.abs(got[:6] - poses[:6]).max() > 1e-3                                      # the window really moved
