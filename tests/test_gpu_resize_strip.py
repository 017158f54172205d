"""The strip form of the pyramid resize (k_resize_strip: plan-time coordinate tables, a rolling two-row cache) against the oracle's pyramid().

The strip form runs for a level when batch x dw x dh >= 1.5 M pixels, and for level 1 whenever level 0 is read in place (every image of a
batched call but the last, which is copied) — so every case is a batched DetectAndCompute call, and the levels are read back with
myslam_orb_debug_readback(what = 0) after the complete call.  Images read in place have no level-0 copy: their levels 1.. are compared, all
levels of the last image.  A batch is a handful of distinct images repeated; the first two images, one in the middle and the last are checked.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAND = 64            # destination rows a wave walks (orb_kernels.hip RS_BAND)
NDISTINCT = 3


def _images(synth, seed, rows, cols):
    return [synth.random_image(seed + i, rows, cols, "noise" if i == 1 else "texture") for i in range(NDISTINCT)]


def _run_and_check(api, oracle, ext, imgs, batch, rows, cols, step, ref, params):
    """one batched call on `ext` over imgs[b % len(imgs)] with row pitch `step`, then the pyramid levels of four images against `ref`"""
    import torch
    stride = rows * step + 5 * (step != cols)            # a pitched batch also gets an odd image stride: in-place rows start at any byte
    buf = np.full(batch * stride + 64, 0xA5, np.uint8)
    for b in range(batch):
        v = buf[b * stride: b * stride + rows * step].reshape(rows, step)
        v[:, :cols] = imgs[b % len(imgs)]
    d = torch.from_numpy(buf).cuda()
    cap = ext.max_keypoints(rows, cols)
    kps = torch.zeros(batch * cap * 28, dtype=torch.uint8, device="cuda"); desc = torch.zeros(batch * cap * 32, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(batch, dtype=torch.int32, device="cuda"); st = torch.ones(batch, dtype=torch.int32, device="cuda")
    ext.set_stream(torch.cuda.current_stream().cuda_stream)
    ext.detect_and_compute_batch(d.data_ptr(), batch, rows, cols, step, stride, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), st.data_ptr(), cap)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    for b in sorted({0, 1, batch // 2, batch - 1}):
        lv = ref[b % len(imgs)]
        for l in range(0 if b == batch - 1 else 1, params.nlevels):
            out = np.zeros(lv[l].shape, np.uint8)
            rc = api.lib().myslam_orb_debug_readback(ext._h, 0, b, l, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes), 0)
            assert rc == 0, rc
            bad = np.argwhere(out != lv[l])
            assert bad.size == 0, (b, l, lv[l].shape, len(bad), bad[:4].tolist())


def _case(api, oracle, synth, rows, cols, batch, nlevels=2, scale=1.2, step=None, seed=100, want_dw=None, want_dh=None):
    params = oracle.params(200, scale, nlevels)
    imgs = _images(synth, seed + rows * 7 + cols, rows, cols)
    ref = [oracle.pyramid(params, im) for im in imgs]
    if want_dw is not None: assert ref[0][1].shape[1] == want_dw, ref[0][1].shape
    if want_dh is not None: assert ref[0][1].shape[0] == want_dh, ref[0][1].shape
    ext = api.ORBextractor(200, scale, nlevels)
    _run_and_check(api, oracle, ext, imgs, batch, rows, cols, step or cols, ref, params)


@pytest.mark.parametrize("cols,dw", [(302, 252), (306, 255), (307, 256), (308, 257), (312, 260), (616, 513), (1241, 1034)])
def test_level1_widths_around_strip_and_dword_boundaries(api, oracle, synth, cols, dw):
    """level-1 widths on both sides of a 256-column strip and of a dword; 1034 = five strips, the last one nearly empty.  80 source rows
    give 67 destination rows: two bands"""
    _case(api, oracle, synth, 80, cols, 4, want_dw=dw)


@pytest.mark.parametrize("rows,dh", [(76, BAND - 1), (77, BAND), (78, BAND + 1), (154, 2 * BAND)])
def test_level1_heights_around_the_band_height(api, oracle, synth, rows, dh):
    _case(api, oracle, synth, rows, 320, 4, want_dh=dh)


def test_last_row_with_both_taps_on_the_last_source_row(api, oracle, synth):
    """scale factors in (1, 1.25] never clamp the last row's lower tap (sy = sh - 2 there); a level of the SAME height as its source does
    (scale_y = 1: sy = sh - 1, the lower tap is clamped onto it).  Scale factor 1.005 at 80 rows: level 1 is 318 x 80"""
    _case(api, oracle, synth, 80, 320, 4, scale=1.005, want_dw=318, want_dh=80)


def test_all_eight_levels_take_the_strip_form(api, oracle, synth):
    """320 x 240 x 256 images: level 7 is 89 x 67 = 1.53 M pixels per batch, so every level's tables are used"""
    params = oracle.params(200, 1.2, 8)
    imgs = _images(synth, 7, 240, 320)
    ref = [oracle.pyramid(params, im) for im in imgs]
    assert 256 * ref[0][7].size >= 1500000
    _run_and_check(api, oracle, api.ORBextractor(200, 1.2, 8), imgs, 256, 240, 320, 320, ref, params)


def test_callers_pitch_not_a_multiple_of_four(api, oracle, synth):
    """level 0 read in place through a row pitch of 311 bytes for 308 columns: the unaligned 8-byte form at the table's offsets"""
    _case(api, oracle, synth, 80, 308, 5, step=311)


def test_two_handles_of_different_sizes_used_alternately(api, oracle, synth):
    """each handle owns its tables: neither a later plan nor the other handle's calls may change them"""
    sizes = [(80, 302), (90, 616)]
    params = oracle.params(200, 1.2, 2)
    exts = [api.ORBextractor(200, 1.2, 2) for _ in sizes]
    imgs = [_images(synth, 40 + i, r, c) for i, (r, c) in enumerate(sizes)]
    ref = [[oracle.pyramid(params, im) for im in ims] for ims in imgs]
    for rep in range(2):
        for i, (r, c) in enumerate(sizes):
            _run_and_check(api, oracle, exts[i], imgs[i], 4, r, c, c, ref[i], params)
