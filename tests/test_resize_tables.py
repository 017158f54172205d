"""Host-only check of the plan-time tables of the strip resize (csrc/resize_tab.h): the column and row records the host builds must be the
coordinates and 11-bit weights of cv::resize INTER_LINEAR.  pyoracle exposes no coordinate function, so the records are compared with a
NumPy restatement of OpenCV's fx = (d + 0.5) * scale - 0.5 (f64 product and difference, f32 from there, nearest-even conversions) — and,
to tie that restatement to the oracle itself, a resize computed from the records alone must equal the oracle's resize() byte for byte.

The header is plain C++: the test compiles a small driver around it with the host compiler (one compile, one run for all sizes)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR

SIZES = [(80, 302), (80, 306), (80, 307), (80, 308), (80, 312), (80, 616), (80, 1241), (76, 320), (77, 320), (78, 320), (154, 320), (240, 320), (376, 1241)]
SCALES = [1.2, 1.25]

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "resize_tab.h"
using namespace myslam_hip;
int main(int argc, char** argv) {          // out.bin, then quadruples sw sh dw dh: per quadruple the column records of whole strips, then the row records
    FILE* f = fopen(argv[1], "wb");
    if (!f) return 1;
    for (int i = 2; i + 3 < argc; i += 4) {
        const int sw = atoi(argv[i]), sh = atoi(argv[i + 1]), dw = atoi(argv[i + 2]), dh = atoi(argv[i + 3]);
        const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);      // level_resize_args, orb_engine.hip
        std::vector<ResizeColRec> c; std::vector<ResizeRowRec> r;
        resize_col_records(sw, dw, scale_x, (dw + 255) / 256 * 64, c);
        resize_row_records(sh, dh, scale_y, r);
        fwrite(c.data(), sizeof(ResizeColRec), c.size(), f);
        fwrite(r.data(), sizeof(ResizeRowRec), r.size(), f);
    }
    return fclose(f) != 0;
}
"""


def _cv_round(v):                       # cvRound((float)v) of a non-negative float: nearest, ties to even
    return np.rint(v).astype(np.int64)


def _coords(ssize, dsize, is_x):
    """OpenCV 3.4 resize.cpp, INTER_LINEAR: source index and the two 11-bit weights of every destination index"""
    scale = 1.0 / (float(dsize) / ssize)
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if is_x:
        lo = s < 0; f[lo] = 0; s[lo] = 0
        hi = s >= ssize - 1; f[hi] = 0; s[hi] = ssize - 1
    c0 = _cv_round(((np.float32(1) - f) * np.float32(2048)).astype(np.float32))
    c1 = _cv_round((f * np.float32(2048)).astype(np.float32))
    return s, c0, c1


@pytest.fixture(scope="module")
def tables(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("resize_tab")
    src = d / "driver.cpp"; exe = d / "driver"; out = d / "out.bin"
    src.write_text(DRIVER)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(PKG_DIR, "csrc"), str(src), "-o", str(exe)], check=True)
    cases = []
    for rows, cols in SIZES:
        for sc in SCALES:
            dw, dh = oracle.level_size(cols, rows, float(np.float32(1.0) / np.float32(sc)))
            cases.append((cols, rows, dw, dh))
    subprocess.run([str(exe), str(out)] + [str(v) for c in cases for v in c], check=True)
    raw = np.fromfile(out, np.uint32)
    res = {}; pos = 0
    for sw, sh, dw, dh in cases:
        ng = (dw + 255) // 256 * 64
        col = raw[pos: pos + 8 * ng].reshape(ng, 8); pos += 8 * ng
        row = raw[pos: pos + 4 * (dh + 2)].reshape(dh + 2, 4); pos += 4 * (dh + 2)
        res[(sw, sh, dw, dh)] = (col, row)
    assert pos == raw.size
    return res


def test_column_records(tables):
    for (sw, sh, dw, dh), (col, _) in tables.items():
        s, c0, c1 = _coords(sw, dw, True)
        d = np.minimum(4 * np.arange(len(col))[:, None] + np.arange(4)[None, :], dw - 1)      # groups past the last column repeat it
        sx = s[d]
        assert np.array_equal(col[:, 0], sx[:, 0]), (sw, dw)
        o = sx - sx[:, :1]
        assert o.min() >= 0 and o.max() <= 6, (sw, dw, o.max())                               # the 8-byte window holds every byte pair
        sel = 0x0C000C00 | ((o + 1) << 16) | o
        assert (sel[:, 0] == 0x0C010C00).all()
        assert np.array_equal(col[:, 1:4], sel[:, 1:]), (sw, dw)
        assert np.array_equal(col[:, 4:8], c0[d] | (c1[d] << 16)), (sw, dw)
        assert (c0[d] + c1[d] == 2048).all()


def test_row_records(tables):
    for (sw, sh, dw, dh), (_, row) in tables.items():
        s, b0, b1 = _coords(sh, dh, False)
        up = np.clip(s, 0, sh - 1); low = np.clip(s + 1, 0, sh - 1)
        assert np.array_equal(row[:dh, 0], up), (sh, dh)
        assert np.array_equal(row[:dh, 1], (up == low).astype(np.uint32)), (sh, dh)
        assert np.array_equal(row[:dh, 2], b0 << 12) and np.array_equal(row[:dh, 3], b1 << 12), (sh, dh)
        assert (row[dh:] == row[dh - 1]).all()                                                # the spare records the walk's look-ahead reads
        assert (np.diff(up) >= 1).all() and up[0] >= 0                                        # what the rolling walk relies on: one step down per destination row at least


def test_resize_from_the_records_is_the_oracles_resize(tables, oracle):
    rng = np.random.default_rng(5)
    for (sw, sh, dw, dh), (col, row) in list(tables.items())[::5]:
        img = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        g = np.arange(dw) // 4; k = np.arange(dw) % 4
        sx = col[g, 0].astype(np.int64) + ((col[g, 1 + np.maximum(k - 1, 0)] & 0xFF) * (k > 0))
        aw = col[g, 4 + k].astype(np.int64)
        a0, a1 = aw & 0xFFFF, aw >> 16
        p = img.astype(np.int64)
        h = p[:, sx] * a0 + p[:, np.minimum(sx + 1, sw - 1)] * a1                               # the row cache (the weight of a column past the row is 0)
        up = row[:dh, 0].astype(np.int64); low = np.where(row[:dh, 1] == 1, up, up + 1)
        b0 = (row[:dh, 2] >> 12).astype(np.int64)[:, None]; b1 = (row[:dh, 3] >> 12).astype(np.int64)[:, None]
        out = (((b0 * (h[up] >> 4)) >> 16) + ((b1 * (h[low] >> 4)) >> 16) + 2) >> 2
        assert np.array_equal(out.astype(np.uint8), oracle.resize(img, dw, dh)), (sw, sh, dw, dh)
