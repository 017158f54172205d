"""numpy float64 restatement of cv::undistort as Camera::UndistortImage calls it (reference src/camera.cpp:36-48): the map of
initUndistortRectifyMap(..., CV_16SC2) per stripe and the fixed-point bilinear remap with border 0.  The C++ twin is
csrc/undistort_map.h (the map) + csrc/undistort.hip (the remap); tests hold the library to this file byte for byte.

Map, per stripe of min(max(1, 4096 // cols), rows) rows starting at y: Ar = A with Ar(1,2) = cy - y, iR = Ar^-1 by the 3 x 3 cofactor
formula; row i of the stripe starts at (_x, _y, _w) = i * (ir1, ir4, ir7) + (ir2, ir5, ir8) and adds (ir0, ir3, ir6) after every column
(np.add.accumulate adds in order).  cvRound = np.rint (half to even), then arithmetic shifts and a wrap to int16."""
import numpy as np


def stripe_rows(rows, cols):
    return min(max(1, 4096 // max(cols, 1)), rows)


def _inv3(a):
    """Mat::inv(DECOMP_LU) for 3 x 3: det3, d = 1 / det, b(i, j) = cofactor * d"""
    d = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + \
        a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0])
    d = 1.0 / d
    return [(a[1][1] * a[2][2] - a[1][2] * a[2][1]) * d, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * d, (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * d,
            (a[1][2] * a[2][0] - a[1][0] * a[2][2]) * d, (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * d, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * d,
            (a[1][0] * a[2][1] - a[1][1] * a[2][0]) * d, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * d, (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * d]


def _cv_round(v):
    """cvRound(double) on x86: half to even; outside int (or NaN) gives INT_MIN"""
    ok = (v >= -2147483648.5) & (v < 2147483647.5)
    return np.where(ok, np.rint(np.where(ok, v, 0.0)), -2147483648.0).astype(np.int64)


def undistort_maps(rows, cols, K, D):
    """OpenCV's two maps: xy (rows, cols, 2) int16 and frac (rows, cols) uint16.  K = (fx, fy, cx, cy), D = (k1, k2, p1, p2), both taken
    through float32 first (the reference holds them as float)."""
    fx, fy, u0, v0 = (float(np.float32(k)) for k in K)
    k1, k2, p1, p2 = (float(np.float32(k)) for k in D)
    k3 = k4 = k5 = k6 = s1 = s2 = s3 = s4 = 0.0
    xy = np.zeros((rows, cols, 2), np.int16); frac = np.zeros((rows, cols), np.uint16)
    s0 = stripe_rows(rows, cols)
    for y in range(0, rows, s0):
        n = min(s0, rows - y)
        ir = _inv3([[fx, 0.0, u0], [0.0, fy, v0 - float(y)], [0.0, 0.0, 1.0]])
        i = np.arange(n, dtype=np.float64)[:, None]

        def run(step, a, b):
            v = np.empty((n, cols), np.float64)
            v[:, :] = step
            v[:, 0:1] = i * a + b
            return np.add.accumulate(v, axis=1)
        _x, _y, _w = run(ir[0], ir[1], ir[2]), run(ir[3], ir[4], ir[5]), run(ir[6], ir[7], ir[8])
        w = 1.0 / _w
        x = _x * w; yy = _y * w
        x2 = x * x; y2 = yy * yy
        r2 = x2 + y2; _2xy = 2 * x * yy
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2
        yd = yy * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
        u = fx * xd + u0; v = fy * yd + v0
        iu = _cv_round(u * 32); iv = _cv_round(v * 32)
        xy[y:y + n, :, 0] = ((iu >> 5) & 0xFFFF).astype(np.uint16).view(np.int16)
        xy[y:y + n, :, 1] = ((iv >> 5) & 0xFFFF).astype(np.uint16).view(np.int16)
        frac[y:y + n] = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return xy, frac


def remap(src, xy, frac):
    """remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) for 8-bit images: weights (32 - fx)(32 - fy) 32 ... (sum 32768), a corner
    outside the image reads 0, out = (sum + 16384) >> 15"""
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    sx = xy[..., 0].astype(np.int64); sy = xy[..., 1].astype(np.int64)
    fx = (frac & 31).astype(np.int64); fy = ((frac >> 5) & 31).astype(np.int64)

    def at(x, y):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), 0)
    s = (at(sx, sy) * ((32 - fx) * (32 - fy) * 32) + at(sx + 1, sy) * (fx * (32 - fy) * 32) +
         at(sx, sy + 1) * ((32 - fx) * fy * 32) + at(sx + 1, sy + 1) * (fx * fy * 32))
    return ((s + 16384) >> 15).astype(np.uint8)


def undistort(src, K, D):
    """cv::undistort(src, dst, K, D) — the stripes only reset the map's row origin, so one whole-image map gives the same bytes"""
    src = np.asarray(src, np.uint8)
    xy, frac = undistort_maps(src.shape[0], src.shape[1], K, D)
    return remap(src, xy, frac)
