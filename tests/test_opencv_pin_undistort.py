"""cv::undistort as Camera::UndistortImage calls it (reference src/camera.cpp:36-48) against OpenCV itself, through the fixture
tools/dump_opencv_goldens.py writes on a machine that has OpenCV (tests/golden/opencv_undistort.npz).  Without it every test reports
    XFAIL  parity unpinned: ...
as tests/test_opencv_pin.py does.  A mismatch names what to change first: the running-sum form of initUndistortRectifyMap's line loop
(an AVX2 build may compute base + j * ir[0]) in tests/undistort_ref.py and csrc/undistort_map.h."""
import numpy as np
import pytest

import undistort_ref as U
from test_opencv_pin import fixture


@pytest.mark.parametrize("name", ["mild", "strong"])
def test_undistort_output(name):
    f = fixture("opencv_undistort.npz")
    K = f["K"]
    got = U.undistort(f["src"], (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), f[f"{name}_D"])
    assert np.array_equal(got, f[f"{name}_out"]), (f"cv::undistort ({name}) differs from tests/undistort_ref.py (OpenCV {f['version']}): "
                                                   "check the map first (test_undistort_stripe_map)")


@pytest.mark.parametrize("name", ["mild", "strong"])
def test_undistort_stripe_map(name):
    f = fixture("opencv_undistort.npz")
    K = f["K"]; src = f["src"]
    y0 = int(f[f"{name}_stripe_y0"]); want_xy, want_frac = f[f"{name}_map_xy"], f[f"{name}_map_frac"]
    xy, frac = U.undistort_maps(src.shape[0], src.shape[1], (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), f[f"{name}_D"])
    n = want_xy.shape[0]
    assert np.array_equal(xy[y0:y0 + n], want_xy) and np.array_equal(frac[y0:y0 + n], want_frac), \
        (f"initUndistortRectifyMap ({name}) differs (OpenCV {f['version']}): try base + j * ir[0] in place of the running sums")
