"""Inputs shared by the LK edge tests (tests/test_gpu_lk_edges.py, tests/test_oracle_kat.py).  Test infrastructure: plain numpy, no oracle and no
product code, so that the preconditions the tests assert (window sums beyond 32 bits) are computed independently of both."""
import numpy as np

# the coordinates no image holds: non-finite, far outside the int range, and the floats at its two ends
NON_FINITE = [np.nan, np.inf, -np.inf]
OUT_OF_RANGE = [1e10, -1e10, 3e9, 2147483648.0, -2147483648.0]


def saturated_pattern(h=120, w=160):
    """vertical stripes 0, 0, 255, 255 (the largest Scharr x-derivative an 8-bit image has: |Ix| = 4080 on every pixel); the rows with
    (y // 2) % 2 == 1 are remapped 0 -> 40, 255 -> 215 so that Iy is not zero everywhere and the 2x2 normal matrix is regular"""
    img = np.tile(np.array([0, 0, 255, 255], np.uint8), (h, (w + 3) // 4))[:, :w].copy()
    rows = (np.arange(h) // 2) % 2 == 1
    img[rows] = np.where(img[rows] == 255, 215, 40).astype(np.uint8)
    return np.ascontiguousarray(img)


def scharr_x(img):
    """3 / 10 / 3 Scharr x-derivative of every pixel, int64, REFLECT_101 neighbours (numpy's "reflect")"""
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    d = p[:, 2:] - p[:, :-2]
    return 3 * d[:-2] + 10 * d[1:-1] + 3 * d[2:]


def window_sums(prev, nxt, x, y, win):
    """(sum Ix^2, sum diff * Ix) in int64 over the win x win window centred on the INTEGER point (x, y) of `prev`, with `nxt` sampled at the same
    point (the first iteration when the initial guess is the point itself).  At an integer point the bilinear weights are (1, 0, 0, 0): the
    template is 32 * pixel, the derivative is the Scharr value, diff = 32 * (nxt - prev).  The window must lie inside the image."""
    r = (win - 1) // 2
    assert r <= x < prev.shape[1] - r and r <= y < prev.shape[0] - r
    sl = (slice(y - r, y + r + 1), slice(x - r, x + r + 1))
    ix = scharr_x(prev)[sl]
    diff = 32 * (nxt.astype(np.int64)[sl] - prev.astype(np.int64)[sl])
    return int((ix * ix).sum()), int((diff * ix).sum())
