"""The ORB extractor on the hand-made inputs of tests/orb_cases.py (FAST scores at the thresholds and at the top of a byte, ring runs of 8 and 9,
equal scores and cell seams, oct-tree split lines / budgets / ties, angles on the axes, BRIEF coordinates half-way between two pixels) against the
CPU oracle, bit-exact: the 28 bytes of every key-point and the 32 of every descriptor.  tests/test_orb_cases.py proves on the oracle alone that
every case reaches its regime.  Every case runs through each code form that has kernels of its own:

  single image     DetectAndCompute, Detect and debug_candidates with FAST_MODE 0 (two-phase) and 1 (dense)           test_single_image
  batch < 64       the 512-thread oct-tree; level 0 read in place and copied (COPY_INPUT 0 / 1)                        test_small_batch
  batch >= 64      the 256-thread oct-tree and the tile-ordered descriptor pass: 64 images per configuration           test_large_batch
  both Gaussians   BLUR_MFMA 0 / 1 on the orientation and descriptor cases                                             test_blur_forms
  second forms     ScreenAndComputeKPsParams + CalcDescriptors (wave_ic_angle, wave_brief), CalcDescriptors with the   test_screen_and_calc_descriptors,
                   bare tie angles, and process_keyframes_batch on the same key-frames                                 test_calc_descriptors_tie_angles,
                                                                                                                       test_process_keyframes_batch"""
import numpy as np
import pytest

import orb_cases as oc

pytestmark = pytest.mark.gpu

CASES = oc.all_cases()
STAMPED = [c for c in CASES if c.regime in ("axis", "ties")]
STAMPED_BY_CONFIG = {}
for _c in STAMPED:
    STAMPED_BY_CONFIG.setdefault(_c.config, []).append(_c)
_cache = {}


def _want(oracle, img, config):
    """(key-points, descriptors) of the oracle, computed once per image and configuration"""
    key = ("dac", img.tobytes(), img.shape, config)
    if key not in _cache:
        _cache[key] = oracle.detect_and_compute(oracle.params(*config), img)
    return _cache[key]


def _explain(a, b):
    n = min(len(a), len(b))
    bad = {f: int((a[f][:n].view(np.int32) != b[f][:n].view(np.int32)).sum()) for f in a.dtype.names}
    first = next((i for i in range(n) if a[i].tobytes() != b[i].tobytes()), None)
    return f"n: {len(a)} vs {len(b)}; fields differing: { {f: k for f, k in bad.items() if k} }; first: {None if first is None else (a[first], b[first])}"


def _assert_same(got, want, tag):
    gk, gd = got
    wk, wd = want
    assert gk.tobytes() == wk.tobytes(), (tag, _explain(gk, wk))
    assert np.array_equal(gd, wd), (tag, f"{int((gd != wd).any(1).sum())} of {len(wd)} descriptors differ, first at {np.nonzero((gd != wd).any(1))[0][:3].tolist()}")


# ------------------------------------------------------------------------------------------------------------------------ single image
@pytest.mark.parametrize("fast_mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_single_image(api, oracle, case, fast_mode):
    ext = case.extractor(api)
    ext.set_option(ext.OPT_FAST_MODE, fast_mode)
    pyr = oracle.pyramid(case.params(oracle), case.img)
    for level in range(case.nlevels):                                   # FAST stage: the candidate set before the oct-tree
        xs, ys, sc = ext.debug_candidates(case.img, level)
        got = sorted(zip(xs.tolist(), ys.tolist(), sc.tolist()))
        rx, ry, rs = oracle.grid_fast(pyr[level], case.ini, case.mn)
        want = sorted(zip(rx.tolist(), ry.tolist(), rs.tolist()))
        assert got == want, (case.name, "FAST", level, f"extra {sorted(set(got) - set(want))[:5]}, missing {sorted(set(want) - set(got))[:5]}")
        if level == 0 and "cands" in case.known:
            assert got == sorted(case.known["cands"])
    _assert_same(ext.DetectAndCompute(case.img), _want(oracle, case.img, case.config), (case.name, "DetectAndCompute"))
    k0 = ext.Detect(case.img)
    r0 = oracle.detect(case.params(oracle), case.img)
    assert k0.tobytes() == r0.tobytes(), (case.name, "oct-tree (Detect)", _explain(k0, r0))


@pytest.mark.parametrize("fast_mode", [0, 1])
def test_strip_without_cells(api, oracle, fast_mode):
    """62 x 903 at one level, the smallest image whose plan holds a strip of no cell: the FAST area is 871 px wide, its 29 grid columns of
    ceil(871 / 29) = 31 px overshoot it, the last column starts past the area (ORBextractor.cpp:852 skips it) and is the only cell of the
    row's eighth strip of four — that strip's block of k_fast_strip returns as soon as it has read its record"""
    h, w = 62, 903
    ncols = (w - 32) // 30
    wcell = -(-(w - 32) // ncols)
    assert ncols % 4 == 1 and 16 + (ncols - 1) * wcell >= w - 16 - 6
    img = _fillers(h, w)[1]
    ext = api.ORBextractor(300, 1.2, 1)
    ext.set_option(ext.OPT_FAST_MODE, fast_mode)
    xs, ys, sc = ext.debug_candidates(img, 0)
    rx, ry, rs = oracle.grid_fast(img, 20, 7)
    assert sorted(zip(xs.tolist(), ys.tolist(), sc.tolist())) == sorted(zip(rx.tolist(), ry.tolist(), rs.tolist())) and len(rx) > 0
    _assert_same(ext.DetectAndCompute(img), _want(oracle, img, (300, 1.2, 1, 20, 7)), "DetectAndCompute")


# ------------------------------------------------------------------------------------------------------------------------ batches
def _fillers(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    return np.full((h, w), 90, np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)


def _run_batch(api, ext, imgs):
    import torch
    B, (h, w) = len(imgs), imgs[0].shape
    cap = ext.max_keypoints(h, w)
    d_imgs = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).cuda()
    d_kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda"); d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(B, dtype=torch.int32, device="cuda"); d_st = torch.ones(B, dtype=torch.int32, device="cuda")
    ext.set_stream(torch.cuda.current_stream().cuda_stream)
    ext.detect_and_compute_batch(d_imgs.data_ptr(), B, h, w, w, h * w, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), d_st.data_ptr(), cap)
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert (d_st.cpu().numpy() == 0).all() and (cnt <= cap).all()
    kps = d_kps.cpu().numpy().view(api.KP_DTYPE).reshape(B, cap); desc = d_desc.cpu().numpy().reshape(B, cap, 32)
    return [(kps[b, :cnt[b]], desc[b, :cnt[b]]) for b in range(B)]


def _groups():
    g = {}
    for c in CASES:
        g.setdefault((c.img.shape, c.config), []).append(c)
    return g


@pytest.mark.parametrize("copy_input", [0, 1])
def test_small_batch(api, oracle, copy_input):
    """every case among the cases of its own configuration, between a flat and a noise image: fewer than 64 images, so k_octree<512>"""
    for (shape, config), cases in _groups().items():
        flat, noise = _fillers(*shape)
        imgs = [flat] + [c.img for c in cases] + [noise]
        assert len(imgs) < 64
        ext = cases[0].extractor(api)
        ext.set_option(ext.OPT_COPY_INPUT, copy_input)
        for rep in range(2):                                             # the second call takes the FAST path the first one's statistics choose
            got = _run_batch(api, ext, imgs)
            for b, img in enumerate(imgs):
                _assert_same(got[b], _want(oracle, img, config), (config, copy_input, rep, b, cases[b - 1].name if 0 < b <= len(cases) else "filler"))


GROUPS = _groups()


@pytest.mark.parametrize("group", list(GROUPS), ids=lambda g: "%dx%d-%s" % (g[0] + (g[1],)))
def test_large_batch(api, oracle, group):
    """every case in a call of 64 images under its OWN configuration (budget, levels, thresholds): k_octree<256> and the tile-ordered descriptor
    pass.  The batch is the group's case images, a flat and a noise image, repeated until it holds 64: every case sits at several batch positions."""
    shape, config = group
    cases = GROUPS[group]
    flat, noise = _fillers(*shape)
    unit = [(c.name, c.img) for c in cases] + [("flat", flat), ("noise", noise)]
    named = [unit[i % len(unit)] for i in range(64)]
    ext = cases[0].extractor(api)
    got = _run_batch(api, ext, [im for _, im in named])
    for b, (name, img) in enumerate(named):
        _assert_same(got[b], _want(oracle, img, config), (config, b, name))


# ------------------------------------------------------------------------------------------------------------------------ both Gaussian forms
@pytest.mark.parametrize("config", list(STAMPED_BY_CONFIG), ids=str)
@pytest.mark.parametrize("mfma", [0, 1])
def test_blur_forms(api, oracle, mfma, config):
    cases = STAMPED_BY_CONFIG[config]
    ext = cases[0].extractor(api)
    ext.set_option(ext.OPT_BLUR_MFMA, mfma)
    for c in cases:
        _assert_same(ext.DetectAndCompute(c.img), _want(oracle, c.img, config), (c.name, mfma))
        pyr = oracle.pyramid(c.params(oracle), c.img)
        for level in range(c.nlevels):
            assert np.array_equal(ext.debug_pyramid(c.img, level, blurred=True), oracle.blur7(pyr[level], 0)), (c.name, mfma, level)
    got = _run_batch(api, ext, [c.img for c in cases])
    for b, c in enumerate(cases):
        _assert_same(got[b], _want(oracle, c.img, config), (c.name, mfma, "batch"))


# ------------------------------------------------------------------------------------------------------------------------ the second implementations
@pytest.mark.parametrize("case", STAMPED, ids=repr)
def test_screen_and_calc_descriptors(api, oracle, case):
    """k_screen (wave_ic_angle) and CalcDescriptors (wave_brief) on the key-points the oracle detected, every level: the angles on the axes and
    the half-way coordinates meet the one-wave-per-key-point forms"""
    p = case.params(oracle)
    kin, _ = _want(oracle, case.img, case.config)
    ext = case.extractor(api)
    out, _ = ext.ScreenAndComputeKPsParams(case.img, kin)
    rout = oracle.screen(p, case.img, kin)
    assert out.tobytes() == rout.tobytes(), (case.name, _explain(out, rout))
    assert (rout["octave"] == 0).sum() == (kin["octave"] == 0).sum() > 0
    d = ext.CalcDescriptors(case.img, out)
    rd = oracle.calc_descriptors(p, case.img, rout)
    assert np.array_equal(d, rd), (case.name, f"{int((d != rd).any(1).sum())} of {len(d)} descriptors differ")


def test_calc_descriptors_tie_angles(api, oracle):
    """CalcDescriptors takes the caller's angle: the bare angles with the most half-way coordinates, on three levels of a noise image"""
    img, kps = oc.tie_angle_keypoints(api.KP_DTYPE)
    ext = api.ORBextractor(oc.TIE_NFEATURES, 1.2, 3)
    d = ext.CalcDescriptors(img, kps)
    rd = oracle.calc_descriptors(oracle.params(oc.TIE_NFEATURES, 1.2, 3), img, kps)
    assert np.array_equal(d, rd), f"descriptors differ at {np.nonzero((d != rd).any(1))[0].tolist()}: angles {[float(kps[i]['angle']) for i in np.nonzero((d != rd).any(1))[0]]}"


@pytest.mark.parametrize("config", list(STAMPED_BY_CONFIG), ids=str)
def test_process_keyframes_batch(api, oracle, config):
    """myslam_orb_process_keyframes_batch (k_pkf_screen + the batched descriptor pass) with the stamp images as key-frames and their level-0
    key-points as the frontend's features"""
    import torch
    from test_gpu_process_kf import Call, _check_item
    from test_process_kf_ref import reference
    cases = STAMPED_BY_CONFIG[config]
    p = oracle.params(*config)
    imgs = [c.img for c in cases]
    xys = []
    for c in cases:
        k, _ = _want(oracle, c.img, config)
        k = k[k["octave"] == 0]
        xys.append(np.stack([k["x"], k["y"]], 1).astype(np.float32))
    feat_cap = max(len(xy) for xy in xys) + 3
    want = [reference(oracle, p, im, xy) for im, xy in zip(imgs, xys)]
    assert all(len(w[0]) >= len(xy) > 0 for w, xy in zip(want, xys))              # level 0 keeps every feature: they are its FAST corners
    call = Call(torch, api, imgs, oc.W + 8, xys, feat_cap=feat_cap, cap=feat_cap * config[2])
    ext = api.ORBextractor(*config)
    ext.set_stream(torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        call.clear(); call.run(ext)
        r = call.results()
        for b in range(call.B):
            _check_item(r, b, want[b], (cases[b].name, rep))
