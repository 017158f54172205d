"""The LK tracker (csrc/lk.hip) on the inputs the frontend does not send on a good day, against the oracle restatement (oracle/lk_oracle.cpp),
bit for bit: non-finite and out-of-range coordinates, window sums beyond 32 bits, padded rows and image strides, counts above cap, and the
limits myslam_lk_create accepts (seven pyramid levels, windows 3 / 5 / 13, images one pixel high or wide)."""
import ctypes as C

import numpy as np
import pytest

import lk_cases as LC

pytestmark = pytest.mark.gpu


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(g, r, tag=""):
    """(positions, status, err) of the kernel and of the oracle: identical bits"""
    assert np.array_equal(g[1], r[1]), (tag, "status", np.flatnonzero(g[1] != r[1])[:8])
    assert np.array_equal(_u32(g[2]), _u32(r[2])), (tag, "err", np.flatnonzero(_u32(g[2]) != _u32(r[2]))[:8])
    bad = np.flatnonzero((_u32(g[0]) != _u32(r[0])).any(axis=1))
    assert len(bad) == 0, (tag, "positions", bad[:8], g[0][bad[:4]], r[0][bad[:4]])


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------------------------------------- non-finite and out-of-range coordinates
def _hostile_points(w, h):
    """every value of LC.NON_FINITE + LC.OUT_OF_RANGE once in x and once in y of prev_pts, and once in x and once in y of the initial guess: one
    point per (value, slot), point k of them at index 5 k + slot between ordinary points, so that the bad points, and the non-finite ones among
    them, visit all four waves of a block"""
    values = LC.NON_FINITE + LC.OUT_OF_RANGE
    n_bad = 4 * len(values)
    rng = np.random.default_rng(21)
    pts = rng.uniform([12, 12], [w - 12, h - 12], size=(5 * n_bad, 2)).astype(np.float32)
    init = (pts + rng.normal(0, 1.0, size=pts.shape)).astype(np.float32)
    bad = 5 * np.arange(n_bad) + np.repeat(np.arange(4), len(values))
    non_finite = np.zeros(len(pts), bool)
    for slot in range(4):                                        # 0 prev x, 1 prev y, 2 init x, 3 init y
        for vi, v in enumerate(values):
            i = bad[slot * len(values) + vi]
            (pts if slot < 2 else init)[i, slot & 1] = v
            non_finite[i] = not np.isfinite(v)
    assert len(set(bad.tolist())) == n_bad and set((bad % 4).tolist()) == {0, 1, 2, 3} and non_finite.sum() == 4 * len(LC.NON_FINITE)
    for wave in range(4):                                        # each wave of a four-wave block holds a non-finite point at least once
        assert non_finite[wave::4].any()
    return pts, init, non_finite


def _check_hostile(g, r, pts, init, non_finite, tag):
    g_pts, g_st, g_err = g
    r_pts, r_st, r_err = r
    assert np.array_equal(g_st, r_st), (tag, np.flatnonzero(g_st != r_st), pts[g_st != r_st], init[g_st != r_st])
    assert np.array_equal(_u32(g_err), _u32(r_err)), tag
    assert np.array_equal(_u32(g_pts[r_st]), _u32(r_pts[r_st])), tag
    # a point with a non-finite coordinate is lost, with error 0; its position is left unspecified (OpenCV's rule, NaN payloads need not agree)
    assert not g_st[non_finite].any() and not np.any(g_err[non_finite]), tag
    # every other point, lost ones and those far outside the int range included, has the oracle's position bits
    assert np.array_equal(_u32(g_pts[~non_finite]), _u32(r_pts[~non_finite])), tag
    assert np.isfinite(g_pts[g_st]).all(), (tag, "a tracked point has a non-finite position")
    assert r_st.sum() > len(r_st) // 2                            # the ordinary points between them are tracked


def test_lk_non_finite_and_out_of_range_points(api, oracle, synth):
    a = synth.random_image(77, 120, 160); b = np.roll(a, 1, axis=1).copy()
    pts, init, non_finite = _hostile_points(160, 120)
    r = oracle.lk_track(a, b, pts, init)
    assert not r[1][non_finite].any() and not np.any(r[2][non_finite])
    lk = api.LKTracker()
    _check_hostile(lk.track(a, b, pts, init), r, pts, init, non_finite, "track")
    _check_hostile(lk.track_cached(a, 11, b, 12, pts, init), r, pts, init, non_finite, "track_cached")


def test_lk_non_finite_points_batch(api, oracle, synth):
    import torch
    a = synth.random_image(77, 120, 160); b = np.roll(a, 1, axis=1).copy()
    pts, init, non_finite = _hostile_points(160, 120)
    n = len(pts); cap = n + 3                                     # cap is no multiple of the four points of a block
    # pair 1: the images swapped and the points two slots further on, so that the bad points sit in other waves
    P = np.zeros((2, cap, 2), np.float32); I = np.zeros((2, cap, 2), np.float32)
    P[0, :n] = pts; I[0, :n] = init; P[1, :n] = np.roll(pts, 2, axis=0); I[1, :n] = np.roll(init, 2, axis=0)
    nf = [non_finite, np.roll(non_finite, 2)]
    prev = np.stack([a, b]); nxt = np.stack([b, a])
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (prev, nxt, P, I, np.array([n, n], np.int32))]
    st = torch.zeros(2, cap, dtype=torch.uint8, device="cuda"); err = torch.zeros(2, cap, device="cuda")
    lk = api.LKTracker(stream=torch.cuda.current_stream().cuda_stream)
    lk.track_batch(d[0].data_ptr(), d[1].data_ptr(), 2, 120, 160, 160, 120 * 160, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), cap, st.data_ptr(),
                   err.data_ptr())
    torch.cuda.synchronize()
    for k in range(2):
        r = oracle.lk_track(prev[k], nxt[k], P[k, :n], I[k, :n])
        g = (d[3][k, :n].cpu().numpy(), st[k, :n].cpu().numpy().astype(bool), err[k, :n].cpu().numpy())
        _check_hostile(g, r, P[k, :n], I[k, :n], nf[k], f"pair {k}")


# ---------------------------------------------------------------------------------------------- exact window sums beyond 32 bits
def test_lk_window_sums_beyond_32_bits(api, oracle):
    """lk_wave_sum64: on the saturated stripe pattern the exact integer sums of a 15 x 15 window do not fit 32 bits (sum Ix^2, and sum diff * Ix of
    the first iteration against the pattern moved by one pixel).  The preconditions are computed here in int64 with numpy; a kernel that added
    its per-lane partials in one 32-bit pass would lose the top bit and track elsewhere."""
    a = LC.saturated_pattern(120, 160); b = np.roll(a, 1, axis=1).copy()
    grid = [(x, y) for y in (50, 51, 53, 64) for x in (60, 61, 62, 63)]
    sums = {win: [LC.window_sums(a, b, x, y, win) for (x, y) in grid] for win in (13, 15)}
    assert all(s11 > 2 ** 31 for s11, _ in sums[15])              # every 15 x 15 window of the pattern
    assert all(abs(sb) > 2 ** 31 for _, sb in sums[15])
    assert any(abs(sb) > 2 ** 31 for _, sb in sums[13]) and all(s11 < 2 ** 31 for s11, _ in sums[13])      # win 13: only the mismatch vector
    rng = np.random.default_rng(8)
    pts = np.concatenate([np.array(grid, np.float64), rng.uniform([0, 0], [160, 120], size=(150, 2))]).astype(np.float32)
    for win in (13, 15):
        for lv in (0, 2):
            r = oracle.lk_track(a, b, pts, pts, win=win, max_level=lv)
            assert r[1][:len(grid)].all() and np.abs(r[0][:len(grid)] - pts[:len(grid)] - [1.0, 0.0]).max() < 0.01      # the one-pixel move is found
            _assert_same(api.LKTracker(win=win, max_level=lv).track(a, b, pts, pts), r, (win, lv))


# ---------------------------------------------------------------------------------------------- row pitch and image stride
def _padded(img, step, fill):
    """`img` as a view with row pitch `step` into a buffer that ends at the last pixel of the last row; every padding byte = fill"""
    rows, cols = img.shape
    buf = np.full(rows * step - (step - cols), fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (rows, cols), (step, 1))
    view[:] = img
    assert view.strides == (step, 1)
    return buf, view


def _raw_track(api, lk, prev, nxt, pts, init, tokens=None):
    """myslam_lk_track / myslam_lk_prefetch + myslam_lk_track_cached through the C ABI with the views' own row pitches"""
    n = len(pts); npts = init.copy(); st = np.full(n, 0xAA, np.uint8); err = np.full(n, -1.0, np.float32)
    rows, cols = prev.shape
    L = api.lib()
    if tokens is None:
        rc = L.myslam_lk_track(lk._h, _ptr(prev), _ptr(nxt), rows, cols, prev.strides[0], nxt.strides[0], _ptr(pts), _ptr(npts), n, _ptr(st), _ptr(err))
    else:
        rc = L.myslam_lk_prefetch(lk._h, _ptr(nxt), C.c_uint64(tokens[1]), rows, cols, nxt.strides[0])
        assert rc == 0, rc
        rc = L.myslam_lk_track_cached(lk._h, _ptr(prev), C.c_uint64(tokens[0]), _ptr(nxt), C.c_uint64(tokens[1]), rows, cols, prev.strides[0],
                                      nxt.strides[0], _ptr(pts), _ptr(npts), n, _ptr(st), _ptr(err))
    assert rc == 0, rc
    assert set(np.unique(st).tolist()) <= {0, 1}
    return npts, st.astype(bool), err


@pytest.fixture(scope="module")
def pitch_case(oracle, synth):
    a = synth.random_image(997, 97, 131); b = np.roll(a, (1, -2), axis=(0, 1)).copy()
    rng = np.random.default_rng(13)
    pts = np.concatenate([rng.uniform([-4, -4], [135, 101], size=(120, 2)), [[0, 0], [130, 96], [130.5, 0.25], [0.5, 96]]]).astype(np.float32)
    init = (pts + rng.normal(0, 1.0, size=pts.shape)).astype(np.float32)
    return a, b, pts, init, oracle.lk_track(a, b, pts, init)


@pytest.mark.parametrize("pads", [(1, 13), (13, 0), (64, 1)])
def test_lk_row_pitch_host_entries(api, pitch_case, pads):
    """prev_step != next_step != cols, odd pitches; the padding bytes (0 or 255) never reach a result"""
    a, b, pts, init, ref = pitch_case
    assert ref[1].any() and not ref[1].all()
    tok = 1000
    for fill in (0, 255):
        _, va = _padded(a, 131 + pads[0], fill); _, vb = _padded(b, 131 + pads[1], fill)
        lk = api.LKTracker()
        _assert_same(_raw_track(api, lk, va, vb, pts, init), ref, ("track", pads, fill))
        _assert_same(_raw_track(api, lk, va, vb, pts, init, tokens=(tok + 1, tok + 2)), ref, ("cached: prefetch + two misses", pads, fill))
        _assert_same(_raw_track(api, lk, va, vb, pts, init, tokens=(tok + 1, tok + 2)), ref, ("cached: two hits", pads, fill))
        # the same tokens under another pitch name other bytes: found under neither, uploaded again
        _, vb2 = _padded(b, 131 + pads[1] + 3, 255 - fill)
        _assert_same(_raw_track(api, lk, va, vb2, pts, init, tokens=(tok + 1, tok + 2)), ref, ("cached: next under another pitch", pads, fill))
        tok += 10


def test_lk_row_pitch_and_stride_batch(api, pitch_case, oracle):
    """myslam_lk_track_batch with step > cols and stride > rows * step, the images as views into larger device buffers"""
    import torch
    a, b, pts, init, ref = pitch_case
    rows, cols = a.shape; step = cols + 13; stride = rows * step + 77; lead = 19
    B = 2; n = len(pts); cap = n + 1; cnt = np.array([n, n - 7], np.int32)
    imgs_p = [a, b]; imgs_n = [b, a]
    want = [ref, oracle.lk_track(b, a, pts[:n - 7], init[:n - 7])]
    outs = []
    for fill in (0, 255):
        hp = np.full(lead + B * stride, fill, np.uint8); hn = np.full(lead + B * stride, fill, np.uint8)
        for k in range(B):
            for hbuf, img in ((hp, imgs_p[k]), (hn, imgs_n[k])):
                np.lib.stride_tricks.as_strided(hbuf[lead + k * stride:], (rows, cols), (step, 1))[:] = img
        dp = torch.from_numpy(hp).cuda(); dn = torch.from_numpy(hn).cuda()
        P = np.zeros((B, cap, 2), np.float32); I = np.zeros((B, cap, 2), np.float32)
        P[:, :n] = pts; I[:, :n] = init
        d = [torch.from_numpy(x).cuda() for x in (P, I, cnt)]
        st = torch.zeros(B, cap, dtype=torch.uint8, device="cuda"); err = torch.zeros(B, cap, device="cuda")
        lk = api.LKTracker(stream=torch.cuda.current_stream().cuda_stream)
        lk.track_batch(dp.data_ptr() + lead, dn.data_ptr() + lead, B, rows, cols, step, stride, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), cap,
                       st.data_ptr(), err.data_ptr())
        torch.cuda.synchronize()
        for k in range(B):
            m = cnt[k]
            _assert_same((d[1][k, :m].cpu().numpy(), st[k, :m].cpu().numpy().astype(bool), err[k, :m].cpu().numpy()), want[k], ("batch", fill, k))
        outs.append((d[1].cpu().numpy().tobytes(), st.cpu().numpy().tobytes(), err.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


# ---------------------------------------------------------------------------------------------- counts above cap
@pytest.mark.parametrize("counts", [[6, 9, 2], [2, 6, 11]])
def test_lk_counts_above_cap_are_read_as_cap(api, oracle, synth, counts):
    """d_counts[b] > cap with cap % 4 != 0: the waves of slots cap .. cap + 3 must not run (they would work on the next pair's row, and past the
    end of the buffers for the last pair).  Every per-point tensor has one row more than the batch, pre-filled with a sentinel, so a kernel that
    does not clamp lands inside the allocation: [6, 9, 2] sends pair 1 into pair 2's first slots, [2, 6, 11] sends the last pair into the extra row."""
    import torch
    cap, B = 6, 3
    imgs = [synth.random_image(300 + k, 60, 80) for k in range(B + 1)]
    prev = np.stack(imgs); nxt = np.stack([np.roll(im, k + 1, axis=1) for k, im in enumerate(imgs)])
    rng = np.random.default_rng(4)
    P = rng.uniform([12, 12], [68, 48], size=(B + 1, cap, 2)).astype(np.float32)          # real points in every slot: an extra wave would track them
    used = np.zeros((B + 1, cap), bool)
    for k in range(B):
        used[k, :min(counts[k], cap)] = True
    SENT_PT, SENT_ST, SENT_ERR = np.float32(31.5), 0xAA, np.float32(-5.0)
    I = np.where(used[..., None], P, SENT_PT).astype(np.float32)
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (prev, nxt, P, I, np.array(counts, np.int32))]
    st = torch.full((B + 1, cap), SENT_ST, dtype=torch.uint8, device="cuda"); err = torch.full((B + 1, cap), float(SENT_ERR), device="cuda")
    lk = api.LKTracker(stream=torch.cuda.current_stream().cuda_stream)
    lk.track_batch(d[0].data_ptr(), d[1].data_ptr(), B, 60, 80, 80, 60 * 80, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), cap, st.data_ptr(), err.data_ptr())
    torch.cuda.synchronize()
    g_pts, g_st, g_err = d[3].cpu().numpy(), st.cpu().numpy(), err.cpu().numpy()
    assert np.array_equal(d[2].cpu().numpy(), P)
    # slots past the count in every row, and the whole extra row: untouched
    assert (g_st[~used] == SENT_ST).all(), np.argwhere(g_st != np.where(used, g_st, SENT_ST))
    assert (g_err[~used] == SENT_ERR).all() and (g_pts[~used] == SENT_PT).all()
    for k in range(B):
        m = min(counts[k], cap)
        r = oracle.lk_track(prev[k], nxt[k], P[k, :m], P[k, :m])
        assert r[1].any()
        assert set(np.unique(g_st[k, :m]).tolist()) <= {0, 1}
        _assert_same((g_pts[k, :m], g_st[k, :m].astype(bool), g_err[k, :m]), r, ("pair", k))


# ---------------------------------------------------------------------------------------------- the limits myslam_lk_create accepts
def _levels(rows, cols, win, max_level):
    """top pyramid level (buildOpticalFlowPyramid: stop when the next level would not be larger than the window)"""
    w, h = cols, rows
    for l in range(max_level + 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            return l
    return max_level


def _scatter(rng, rows, cols, n):
    pts = rng.uniform([-3, -3], [cols + 3, rows + 3], size=(n, 2)).astype(np.float32)
    return pts, (pts + rng.normal(0, 0.8, size=pts.shape)).astype(np.float32)


@pytest.mark.parametrize("win,rows,cols,top", [(3, 260, 300, 6), (5, 260, 300, 5), (5, 324, 328, 6)])
def test_lk_seven_pyramid_levels_small_windows(api, oracle, synth, win, rows, cols, top):
    """max_level = LK_MAXL = 6 with the windows of one window pixel per lane.  260 x 300 carries seven levels for win 3 (the top one is 5 x 5) and six
    for win 5; 324 x 328 carries seven for win 5 (top 6 x 6)."""
    assert _levels(rows, cols, win, 6) == top
    a = synth.random_image(500 + win, rows, cols); b = np.roll(a, (-1, 2), axis=(0, 1)).copy()
    pts, init = _scatter(np.random.default_rng(win), rows, cols, 200)
    r = oracle.lk_track(a, b, pts, init, win=win, max_level=6, return_levels=True)
    assert r[3] == top and r[1].any()
    if top == 6:                                                  # the seventh level takes part: without it other tracks come out
        r5 = oracle.lk_track(a, b, pts, init, win=win, max_level=5)
        assert not np.array_equal(_u32(r5[0]), _u32(r[0]))
    _assert_same(api.LKTracker(win=win, max_level=6).track(a, b, pts, init), r[:3], (win, rows, cols))


def test_lk_window_13(api, oracle, synth):
    """three window pixels per lane (169 = 2 * 64 + 41)"""
    a = synth.random_image(913, 97, 131); b = np.roll(a, (1, -2), axis=(0, 1)).copy()
    pts, init = _scatter(np.random.default_rng(13), 97, 131, 200)
    r = oracle.lk_track(a, b, pts, init, win=13, max_level=3)
    assert r[1].any()
    _assert_same(api.LKTracker(win=13, max_level=3).track(a, b, pts, init), r)


@pytest.mark.parametrize("rows,cols,top", [(1, 64, 0), (64, 1, 0), (12, 200, 0), (23, 23, 1)])
def test_lk_degenerate_image_sizes(api, oracle, synth, rows, cols, top):
    """images one pixel high or wide (REFLECT_101 of a single row or column) and images on which the pyramid stops at level 0 or 1, win 11"""
    assert _levels(rows, cols, 11, 3) == top
    a = synth.random_image(700 + rows, rows, cols); b = np.roll(a, (int(rows > 1), int(cols > 1)), axis=(0, 1)).copy()
    rng = np.random.default_rng(rows * 1000 + cols)
    pts, init = _scatter(rng, rows, cols, 90)
    on = np.array([[0, 0], [cols - 1, rows - 1], [(cols - 1) / 2, (rows - 1) / 2], [cols // 3, 0], [0, rows // 3], [cols - 1, 0.25], [0.25, rows - 1]], np.float32)
    pts = np.concatenate([pts, on]); init = np.concatenate([init, on + np.float32(0.5)])
    r = oracle.lk_track(a, b, pts, init, win=11, max_level=3, return_levels=True)
    assert r[3] == top
    _assert_same(api.LKTracker(win=11, max_level=3).track(a, b, pts, init), r[:3], (rows, cols))
    if min(rows, cols) > 1:
        assert r[1].any()
