"""Known-answer checks of the numpy restatement of cv::undistort (tests/undistort_ref.py) — the yardstick the library's undistortion
(csrc/undistort.hip, tests/test_gpu_undistort.py) is held to byte for byte.  CPU only."""
import numpy as np
import pytest

import undistort_ref as U

K = (718.856, 718.856, 607.1928, 185.2157)
STRONG = (-0.28, 0.07, 2e-4, 2e-5)
MILD = (-0.05, 0.01, 1e-4, -5e-5)


def _forward(rows, cols, K, D):
    """the lens model written plainly: pixel (u, v) of the undistorted image shows the source point fx * distort((u - cx) / fx, ...) + cx"""
    fx, fy, cx, cy = (float(np.float32(k)) for k in K)
    k1, k2, p1, p2 = (float(np.float32(k)) for k in D)
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def _map_points(xy, frac):
    return xy[..., 0] + (frac & 31) / 32.0, xy[..., 1] + ((frac >> 5) & 31) / 32.0


def test_stripes_of_the_reference_size():
    assert U.stripe_rows(376, 1241) == 3 and U.stripe_rows(2, 5000) == 1 and U.stripe_rows(2, 100) == 2


@pytest.mark.parametrize("shape", [(376, 1241), (121, 333), (7, 5000)])
def test_zero_coefficients_give_an_integer_map_and_an_exact_copy(shape):
    rows, cols = shape
    xy, frac = U.undistort_maps(rows, cols, K, (0, 0, 0, 0))
    v, u = np.mgrid[0:rows, 0:cols]
    assert not frac.any() and np.array_equal(xy[..., 0], u) and np.array_equal(xy[..., 1], v)
    img = np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(U.undistort(img, K, (0, 0, 0, 0)), img)


@pytest.mark.parametrize("D", [MILD, STRONG])
def test_map_within_a_32nd_of_a_pixel_of_the_lens_model(D):
    rows, cols = 376, 1241
    mx, my = _map_points(*U.undistort_maps(rows, cols, K, D))
    fx, fy = _forward(rows, cols, K, D)
    assert np.abs(mx - fx).max() <= 1 / 64 + 1e-6 and np.abs(my - fy).max() <= 1 / 64 + 1e-6


@pytest.mark.parametrize("D", [MILD, STRONG])
def test_map_inverts_to_the_pixel_grid_solved_by_scipy(D):
    """scipy solves distort(q) = map point for q; q lands on the output pixel within 1/32 px"""
    from scipy.optimize import least_squares
    rows, cols = 376, 1241
    mx, my = _map_points(*U.undistort_maps(rows, cols, K, D))
    fx, fy, cx, cy = (float(np.float32(k)) for k in K)
    k1, k2, p1, p2 = (float(np.float32(k)) for k in D)
    rng = np.random.default_rng(7)
    for v, u in zip(rng.integers(0, rows, 60), rng.integers(0, cols, 60)):
        target = np.array([(mx[v, u] - cx) / fx, (my[v, u] - cy) / fy])

        def res(q):
            x, y = q
            r2 = x * x + y * y
            rad = 1 + k1 * r2 + k2 * r2 * r2
            return np.array([x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y]) - target
        q = least_squares(res, target, xtol=1e-15, ftol=1e-15, gtol=1e-15).x
        assert abs(q[0] * fx + cx - u) < 1 / 32 and abs(q[1] * fy + cy - v) < 1 / 32, (u, v, q)


@pytest.mark.parametrize("D", [MILD, STRONG])
def test_remap_matches_scipy_bilinear_inside_the_image(D):
    from scipy.ndimage import map_coordinates
    rows, cols = 376, 1241
    img = np.random.default_rng(3).integers(0, 256, (rows, cols), dtype=np.uint8)
    xy, frac = U.undistort_maps(rows, cols, K, D)
    mx, my = _map_points(xy, frac)
    ref = map_coordinates(img.astype(np.float64), [my, mx], order=1, mode="constant", cval=0.0)
    got = U.remap(img, xy, frac)
    inside = (xy[..., 0] >= 0) & (xy[..., 0] < cols - 1) & (xy[..., 1] >= 0) & (xy[..., 1] < rows - 1)
    assert inside.mean() > 0.99
    assert np.abs(got[inside].astype(np.float64) - ref[inside]).max() <= 1.0


def test_remap_border_reads_zero():
    img = np.full((4, 6), 200, np.uint8)
    xy = np.zeros((1, 4, 2), np.int16); frac = np.zeros((1, 4), np.uint16)
    xy[0, :, 0] = [-2, -1, 5, 6]; frac[0, :] = 16                      # half a pixel right of each
    out = U.remap(img, xy, frac)
    assert out.tolist() == [[0, 100, 100, 0]]
