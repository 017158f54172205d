// undistort_map.h — the per-camera map of cv::undistort, built on the host in f64 (csrc/undistort.hip uploads it).
//
// Camera::UndistortImage (src/camera.cpp:36-48) is cv::undistort(src, dst, K, D) with K widened from the float members fx_ fy_ cx_ cy_ and
// D = (k1, k2, p1, p2).  OpenCV 3.4 cv::undistort works in stripes of min(max(1, 4096 / cols), rows) rows: for the stripe at row y it sets
// Ar(1,2) = cy - y, inverts Ar by the 3 x 3 cofactor formula (Mat::inv(DECOMP_LU)), calls initUndistortRectifyMap(..., CV_16SC2) on the
// stripe and remaps it (INTER_LINEAR, BORDER_CONSTANT 0).  This file restates the map of every stripe: the scalar line loop of
// initUndistortRectifyMap (running sums _x += ir[0] along the row; an AVX2 build of OpenCV may compute base + j * ir[0] instead, which can move
// a few pixels by 1/32 — the first thing to change if the pin kit, tools/dump_opencv_goldens.py, disagrees), cvRound = round half to even,
// map1 = (short)(iu >> 5), (short)(iv >> 5), map2 = (iv & 31) * 32 + (iu & 31).  tests/undistort_ref.py is the numpy twin.
// Compiled with -ffp-contract=off (build.py EXACT): every product and sum below is rounded on its own, as OpenCV's are.
#pragma once
#include <stdint.h>
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

namespace myslam_hip {

// cvRound(double) on x86: round half to even; a value outside int (or NaN) gives INT_MIN as cvtsd2si does
static inline int ud_cv_round(double v) {
    return (v >= -2147483648.5 && v < 2147483647.5) ? (int)nearbyint(v) : INT_MIN;
}

// OpenCV's two maps for the whole image: xy = rows x cols x 2 (CV_16SC2), frac = rows x cols (CV_16UC1)
static inline void ud_build_cv_maps(int rows, int cols, const float K[4], const float D[4], std::vector<int16_t>& xy, std::vector<uint16_t>& frac) {
    xy.assign((size_t)rows * cols * 2, 0); frac.assign((size_t)rows * cols, 0);
    const double fx = (double)K[0], fy = (double)K[1], u0 = (double)K[2], v0 = (double)K[3];
    const double k1 = (double)D[0], k2 = (double)D[1], p1 = (double)D[2], p2 = (double)D[3];
    const double k3 = 0, k4 = 0, k5 = 0, k6 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    const int stripe0 = std::min(std::max(1, 4096 / std::max(cols, 1)), rows);
    for (int y = 0; y < rows; y += stripe0) {
        const int ssz = std::min(stripe0, rows - y);
        // Ar = A with Ar(1,2) = v0 - y; iR = (Ar * I).inv(DECOMP_LU): OpenCV's closed form for 3 x 3 (det3, then cofactors * (1 / det))
        double a[3][3] = {{fx, 0, u0}, {0, fy, v0 - (double)y}, {0, 0, 1}};
        double d = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                   a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
        d = 1. / d;
        const double ir[9] = {
            (a[1][1] * a[2][2] - a[1][2] * a[2][1]) * d, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * d, (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * d,
            (a[1][2] * a[2][0] - a[1][0] * a[2][2]) * d, (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * d, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * d,
            (a[1][0] * a[2][1] - a[1][1] * a[2][0]) * d, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * d, (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * d};
        for (int i = 0; i < ssz; i++) {
            int16_t* m1 = xy.data() + (size_t)(y + i) * cols * 2;
            uint16_t* m2 = frac.data() + (size_t)(y + i) * cols;
            double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
            for (int j = 0; j < cols; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
                const double w = 1. / _w, x = _x * w, yy = _y * w;
                const double x2 = x * x, y2 = yy * yy;
                const double r2 = x2 + y2, _2xy = 2 * x * yy;
                const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
                const double xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2);
                const double yd = (yy * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2);
                const double u = fx * xd + u0, v = fy * yd + v0;      // the tilt matrix is the identity: fx * (1 * xd) + u0
                const int iu = ud_cv_round(u * 32), iv = ud_cv_round(v * 32);
                m1[j * 2] = (int16_t)(uint16_t)(uint32_t)(iu >> 5);
                m1[j * 2 + 1] = (int16_t)(uint16_t)(uint32_t)(iv >> 5);
                m2[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
            }
        }
    }
}

// The device form: output tiles of UD_TW columns x th rows; tile t reads the source band [bx0, bx0 + bwp) x [by0, by0 + bh) (bx0 a multiple of 4,
// clipped to the one-pixel zero border [-1, cols] x [-1, rows] that a bilinear footprint can touch), and every pixel of it is ONE word:
// frac (10 bits) | x - bx0 (11 bits) << 10 | y - by0 (11 bits) << 21, or UD_ZERO where all four corners lie outside the image (OpenCV writes
// the border value 0 there).  Pixels of a tile beyond the image are UD_ZERO and never stored.
constexpr int UD_TW = 128;                   // 8 threads x 16 pixels per tile row
constexpr uint32_t UD_ZERO = 0xffffffffu;
struct UdTile { int bx0, by0, bwp, bh; };

// false = some tile's band does not fit `max_band` bytes (or the 11-bit fields) at this tile height
static inline bool ud_pack(int rows, int cols, int th, const std::vector<int16_t>& xy, const std::vector<uint16_t>& frac, size_t max_band,
                           std::vector<uint32_t>& map, std::vector<UdTile>& tiles, size_t& band_bytes) {
    const int tx = (cols + UD_TW - 1) / UD_TW, ty = (rows + th - 1) / th;
    map.assign((size_t)tx * ty * UD_TW * th, UD_ZERO); tiles.assign((size_t)tx * ty, UdTile{0, 0, 0, 0});
    band_bytes = 0;
    for (int t = 0; t < tx * ty; t++) {
        const int ox = (t % tx) * UD_TW, oy = (t / tx) * th;
        int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
        for (int r = oy; r < std::min(rows, oy + th); r++)
            for (int c = ox; c < std::min(cols, ox + UD_TW); c++) {
                const int sx = xy[((size_t)r * cols + c) * 2], sy = xy[((size_t)r * cols + c) * 2 + 1];
                if (sx >= cols || sx + 1 < 0 || sy >= rows || sy + 1 < 0) continue;
                x0 = std::min(x0, sx); x1 = std::max(x1, sx + 1); y0 = std::min(y0, sy); y1 = std::max(y1, sy + 1);
            }
        if (x0 == INT_MAX) continue;                      // every pixel of the tile is 0
        const int bx0 = x0 >= 0 ? (x0 & ~3) : -4;        // x0 >= -1
        const int bwp = (x1 + 1 - bx0 + 3) & ~3, bh = y1 + 1 - y0;
        if (bwp > 2044 || bh > 2047 || (size_t)bwp * bh > max_band) return false;
        band_bytes = std::max(band_bytes, (size_t)bwp * bh);
        tiles[t] = UdTile{bx0, y0, bwp, bh};
        uint32_t* m = map.data() + (size_t)t * UD_TW * th;
        for (int r = oy; r < std::min(rows, oy + th); r++)
            for (int c = ox; c < std::min(cols, ox + UD_TW); c++) {
                const size_t k = (size_t)r * cols + c;
                const int sx = xy[k * 2], sy = xy[k * 2 + 1];
                if (sx >= cols || sx + 1 < 0 || sy >= rows || sy + 1 < 0) continue;
                m[(r - oy) * UD_TW + (c - ox)] = (uint32_t)(frac[k] & 1023) | ((uint32_t)(sx - bx0) << 10) | ((uint32_t)(sy - y0) << 21);
            }
    }
    return true;
}

}  // namespace myslam_hip
