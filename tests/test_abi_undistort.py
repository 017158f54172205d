"""The undistortion entry points of the C ABI (include/myslam_hip.h, csrc/undistort.hip) and the config switch of the two hosts (chain.py,
host/myslam_system.hpp): declared, exported, read from Camera.bNeedUndistortion and the eight coefficients.  CPU only."""
import ctypes
import os

import numpy as np
import pytest

import undistort_ref as U
from conftest import ROOT
from test_abi import _declared

NAMES = ["myslam_undistort_create", "myslam_undistort_destroy", "myslam_undistort_set_stream", "myslam_undistort_image", "myslam_undistort_batch",
         "myslam_undistort_get_map"]


def test_undistort_entry_points_declared_and_exported(pkg):
    names = _declared()
    assert all(n in names for n in NAMES), [n for n in NAMES if n not in names]
    lib = ctypes.CDLL(pkg.build_library())
    assert all(hasattr(lib, n) for n in NAMES)
    protos = pkg.api.header_prototypes()
    assert protos["myslam_undistort_batch"] == ("int", ["ptr", "ptr", "int", "int", "size_t", "ptr", "int", "size_t"])
    assert protos["myslam_undistort_create"] == ("int", ["ptr", "int", "int", "ptr", "ptr"])


def test_facade_and_system_name_the_stage():
    host = os.path.join(ROOT, "a-simple-stereo-slam-system-with-deep-loop-closing_amd", "host")
    assert "class Camera" in open(os.path.join(host, "myslam_hip.hpp")).read()
    sysh = open(os.path.join(host, "myslam_system.hpp")).read()
    assert "Camera.bNeedUndistortion" in sysh and "Camera.left.k1" in sysh and "Camera.right.p2" in sysh


KITTI = {"Camera.right.fx": "718.856", "Camera.right.fy": "718.856", "Camera.right.cx": "607.1928", "Camera.right.cy": "185.2157", "Camera.bf": "386.1448"}
COEF = {"Camera.left.k1": "-0.28", "Camera.left.k2": "0.07", "Camera.left.p1": "0.0002", "Camera.left.p2": "2e-05",
        "Camera.right.k1": "-0.27", "Camera.right.k2": "0.065", "Camera.right.p1": "0.0001", "Camera.right.p2": "-3e-05"}


def test_camera_from_config_reads_the_switch(pkg):
    chain = pkg.chain
    off = chain.camera_from_config(KITTI)
    assert set(off) == {"fx", "fy", "cx", "cy", "bf", "baseline"}
    assert chain.camera_from_config(dict(KITTI, **COEF, **{"Camera.bNeedUndistortion": "0"})) == off
    on = chain.camera_from_config(dict(KITTI, **COEF, **{"Camera.bNeedUndistortion": "1"}))
    assert on["undistort"] is True
    assert on["dist_left"] == tuple(float(np.float32(v)) for v in ("-0.28", "0.07", "0.0002", "2e-05"))
    assert on["dist_right"] == tuple(float(np.float32(v)) for v in ("-0.27", "0.065", "0.0001", "-3e-05"))
    assert {k: on[k] for k in off} == off


class _Recorder:
    """a back end that only records what Chain.grab hands to undistort() before anything else; the tracker is then stopped"""
    def __init__(self, K):
        self.K, self.seen = K, []

    def undistort(self, img, which):
        self.seen.append(which)
        return U.undistort(img, (self.K["fx"], self.K["fy"], self.K["cx"], self.K["cy"]), self.K["dist_right" if which else "dist_left"])


@pytest.mark.parametrize("on", [False, True])
def test_grab_undistorts_both_images_first_only_with_the_switch(pkg, on):
    chain = pkg.chain
    K = chain.camera_from_config(dict(KITTI, **COEF, **{"Camera.bNeedUndistortion": "1" if on else "0"}))
    rng = np.random.default_rng(0)
    L, R = rng.integers(0, 256, (2, 60, 90), dtype=np.uint8)
    be = _Recorder(K)
    c = chain.Chain(be, pkg.api, K, [(L, R)], log=False)
    c.status = chain.LOST                   # grab() returns at once after the images are taken in
    assert c.grab(0) is False
    assert be.seen == ([0, 1] if on else [])
