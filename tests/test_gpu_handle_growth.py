"""One handle driven through growth, shrinking, regrowth and a change of geometry (csrc/dev_mem.h: every handle's device and pinned blocks are
Buf members, every group of blocks behind a logical size grows through regrow): each call of such a sequence returns what the neighbouring test
files hold a fresh handle to — the oracle's bytes for ORB, LK and the undistorter, tests/test_gpu_lcd.py's tolerance for the descriptor — and,
where the kernels and inputs are the same, the bits of a fresh handle's call.  Handles that allocate once (tracker, PnP solver, loop corrector,
loop database and query context) are created, used and destroyed three times over with equal results.  No test runs the device out of memory:
the failure paths are tests/test_dev_mem.py's."""
import numpy as np
import pytest

import tracker_cases as TC
import undistort_ref as U
from test_gpu_lcd import DESC_ATOL
from test_gpu_loop_correct import CAPS, Run
from test_gpu_process_kf import Call, _check_item
from test_process_kf_ref import expand, reference

pytestmark = pytest.mark.gpu

ORB = (300, 1.2, 3)                                       # nfeatures, scale factor, levels
GEOM = [(96, 128), (100, 90)]


def _mask(h, w):
    m = np.full((h, w), 255, np.uint8); m[h // 4:h // 2, w // 3:2 * w // 3] = 0
    return m


def test_orb_handle_through_batches_masks_and_geometries(api, oracle, synth):
    import torch
    p = oracle.params(*ORB)
    imgs = {g: [synth.random_image(40 + 10 * k + i, *g) for i in range(4)] for k, g in enumerate(GEOM)}
    want = {}

    def ref(g, i, masked):
        if (g, i, masked) not in want:
            want[g, i, masked] = oracle.detect_and_compute(p, imgs[g][i], _mask(*g) if masked else None)
        return want[g, i, masked]

    ext = api.ORBextractor(*ORB)
    ext.set_stream(torch.cuda.current_stream().cuda_stream)

    def batch(g, B, masked):
        h, w = g
        cap = ext.max_keypoints(h, w)
        d = torch.from_numpy(np.stack(imgs[g][:B])).cuda()
        dm = torch.from_numpy(np.stack([_mask(h, w)] * B)).cuda() if masked else None
        kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda"); desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(B, dtype=torch.int32, device="cuda"); st = torch.ones(B, dtype=torch.int32, device="cuda")
        ext.detect_and_compute_batch(d.data_ptr(), B, h, w, w, h * w, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), st.data_ptr(), cap,
                                     d_masks=dm.data_ptr() if masked else 0)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all(), (g, B, masked)
        k = kps.cpu().numpy().view(api.KP_DTYPE).reshape(B, cap); dd = desc.cpu().numpy().reshape(B, cap, 32); n = cnt.cpu().numpy()
        for b in range(B):
            rk, rd = ref(g, b, masked)
            assert n[b] == len(rk) and k[b, :n[b]].tobytes() == rk.tobytes() and np.array_equal(dd[b, :n[b]], rd), (g, B, masked, b)

    # the mask block is allocated late (third call), dropped by the growth to four images, allocated again, and all of it once more per geometry
    for g, B, masked in ((GEOM[0], 1, False), (GEOM[0], 3, False), (GEOM[0], 2, True), (GEOM[0], 4, False), (GEOM[0], 4, True),
                         (GEOM[1], 2, False), (GEOM[1], 3, True), (GEOM[0], 3, True), (GEOM[0], 1, False)):
        batch(g, B, masked)
    assert len(ref(GEOM[0], 0, True)[0]) < len(ref(GEOM[0], 0, False)[0]) and len(ref(GEOM[0], 0, False)[0]) > 30      # the inputs are not degenerate

    # the one-frame calls on the same handle: a caller's cap of 64, then the default one
    img = imgs[GEOM[0]][1]
    rk, rd = ref(GEOM[0], 1, False)
    if len(rk) > 64:
        with pytest.raises(api.MyslamError) as e:
            ext.DetectAndCompute(img, cap=64)
        assert e.value.code == api.ERR_CAPACITY
    else:
        k, d = ext.DetectAndCompute(img, cap=64)
        assert k.tobytes() == rk.tobytes() and np.array_equal(d, rd)
    for _ in range(2):                                       # (the second call of a key replays its graph)
        k, d = ext.DetectAndCompute(img)
        assert k.tobytes() == rk.tobytes() and np.array_equal(d, rd)
    rk, rd = ref(GEOM[0], 1, True)
    k, d = ext.DetectAndCompute(img, _mask(*GEOM[0]))
    assert k.tobytes() == rk.tobytes() and np.array_equal(d, rd)

    # the loop-closing pair (tests/test_gpu_orb.py::test_screen_and_calc_descriptors_bitexact): few rows, then more than any call before
    feats = oracle.detect(p, img)
    xy = np.stack([feats["x"], feats["y"]], 1).astype(np.float32)
    assert len(xy) > 40
    for n in (10, len(xy)):
        pyr = expand(api.KP_DTYPE, xy[:n], ORB[2])
        out, _ = ext.ScreenAndComputeKPsParams(img, pyr)
        rout = oracle.screen(p, img, pyr)
        assert out.tobytes() == rout.tobytes() and len(out) >= n
        assert np.array_equal(ext.CalcDescriptors(img, out), oracle.calc_descriptors(p, img, rout))

    # ProcessNewKF's ORB half for one key-frame, then three (tests/test_gpu_process_kf.py)
    h, w = GEOM[0]
    feat_cap = 384
    for B in (1, 3):
        xys = []
        for i in range(B):
            f = oracle.detect(p, imgs[GEOM[0]][i])
            xys.append(np.stack([f["x"], f["y"]], 1).astype(np.float32)[:feat_cap])
        c = Call(torch, api, imgs[GEOM[0]][:B], w, xys, feat_cap=feat_cap, cap=feat_cap * ORB[2])
        c.run(ext)
        r = c.results()
        for b in range(B):
            _check_item(r, b, reference(oracle, p, imgs[GEOM[0]][b], xys[b]), ("process_keyframes", B))
    batch(GEOM[0], 2, True)                                  # and the batch path still stands


@pytest.mark.parametrize("generic", [0, 1])
def test_deeplcd_handle_through_batches_and_source_sizes(api, oracle, synth, generic):
    import torch
    w = synth.calc_weights()
    sizes = [(120, 160), (97, 131)]
    imgs = {s: np.stack([synth.random_image(300 + 10 * k + i, *s) for i in range(3)]) for k, s in enumerate(sizes)}

    def make():
        h = api.DeepLCD(w)
        h.set_option(h.OPT_GENERIC_KERNELS, generic)
        assert h.uses_fused_kernels() == (not generic)
        return h

    def one(h, s):
        return h.calcDescrOriginalImg(imgs[s][0], blur_in_place=False)[0][None]

    def batch(h, s, B):
        d = torch.from_numpy(imgs[s][:B]).cuda(); out = torch.zeros(B, 1064, device="cuda")
        h.describe_batch(d.data_ptr(), B, s[0], s[1], s[1], s[0] * s[1], out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    lcd = make()
    for call, s, B in ((one, sizes[0], 1), (batch, sizes[0], 3), (batch, sizes[1], 3), (one, sizes[1], 1), (batch, sizes[0], 3), (batch, sizes[0], 1),
                       (one, sizes[0], 1)):
        got = call(lcd, s) if call is one else call(lcd, s, B)
        fresh = call(make(), s) if call is one else call(make(), s, B)
        assert np.array_equal(got.view(np.uint32), fresh.view(np.uint32)), (generic, call.__name__, s, B)
        for b in range(B):
            x, _ = oracle.calc_preproc(imgs[s][b])
            assert np.abs(got[b] - oracle.calc_forward(w, x)).max() < DESC_ATOL, (generic, call.__name__, s, B, b)


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def test_lk_handle_through_batches_point_counts_and_sizes(api, oracle, synth):
    import torch
    sizes = [(97, 131), (120, 160)]
    rng = np.random.default_rng(3)
    frames = {}
    for k, (h, w) in enumerate(sizes):
        prev = np.stack([synth.random_image(500 + 10 * k + i, h, w) for i in range(3)])
        frames[h, w] = (prev, np.ascontiguousarray(np.roll(prev, (1, -2), axis=(1, 2))))

    def points(h, w, n):
        pts = rng.uniform([4, 4], [w - 4, h - 4], size=(n, 2)).astype(np.float32)
        return pts, (pts + rng.normal(0, 1.0, pts.shape)).astype(np.float32)

    def make():
        return api.LKTracker(stream=torch.cuda.current_stream().cuda_stream)

    def batch(lk, size, B, pts, init):
        h, w = size
        cap = pts.shape[1]
        prev, nxt = frames[size]
        cnt = np.asarray([cap - 7 * b for b in range(B)], np.int32)
        d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (prev[:B], nxt[:B], pts[:B], init[:B], cnt)]
        st = torch.zeros(B, cap, dtype=torch.uint8, device="cuda"); err = torch.zeros(B, cap, device="cuda")
        lk.track_batch(d[0].data_ptr(), d[1].data_ptr(), B, h, w, w, h * w, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), cap, st.data_ptr(), err.data_ptr())
        torch.cuda.synchronize()
        return [(d[3][b, :cnt[b]].cpu().numpy(), st[b, :cnt[b]].cpu().numpy().astype(bool), err[b, :cnt[b]].cpu().numpy()) for b in range(B)]

    lk = make()
    for size, B in ((sizes[0], 1), (sizes[0], 3), (sizes[0], 1), (sizes[1], 2), (sizes[0], 3)):
        pi = [points(*size, 64) for _ in range(B)]
        pts = np.stack([p[0] for p in pi]); init = np.stack([p[1] for p in pi])
        got = batch(lk, size, B, pts, init); fresh = batch(make(), size, B, pts, init)
        for b in range(B):
            assert _same_bits(got[b], fresh[b]), (size, B, b)
            n = len(got[b][0])
            r_pts, r_st, _ = oracle.lk_track(frames[size][0][b], frames[size][1][b], pts[b, :n], init[b, :n])
            assert np.array_equal(got[b][1], r_st) and np.array_equal(got[b][0].view(np.uint32), r_pts.view(np.uint32)), (size, B, b)

    # the host-pointer calls on the same handle: 10 points then 200; the cached form below and above its 512-point staging floor
    size = sizes[0]
    prev, nxt = frames[size][0][0], frames[size][1][0]
    for cached, n in ((False, 10), (False, 200), (True, 100), (True, 600), (False, 10), (True, 100)):
        pts, init = points(*size, n)
        call = (lambda h: h.track_cached(prev, 11, nxt, 12, pts, init)) if cached else (lambda h: h.track(prev, nxt, pts, init))
        got, fresh = call(lk), call(make())
        assert _same_bits(got, fresh), (cached, n)
        r_pts, r_st, r_err = oracle.lk_track(prev, nxt, pts, init)
        assert np.array_equal(got[1], r_st) and np.array_equal(got[0].view(np.uint32), r_pts.view(np.uint32)), (cached, n)
        assert np.array_equal(got[2].view(np.uint32), r_err.view(np.uint32)), (cached, n)
    other = sizes[1]                                         # another geometry through the cache, then the first one again
    pts, init = points(*other, 100)
    got = lk.track_cached(frames[other][0][0], 21, frames[other][1][0], 22, pts, init)
    r = oracle.lk_track(frames[other][0][0], frames[other][1][0], pts, init)
    assert np.array_equal(got[1], r[1]) and np.array_equal(got[0].view(np.uint32), r[0].view(np.uint32))
    pts, init = points(*size, 100)
    got = lk.track_cached(prev, 11, nxt, 12, pts, init)
    r = oracle.lk_track(prev, nxt, pts, init)
    assert np.array_equal(got[1], r[1]) and np.array_equal(got[0].view(np.uint32), r[0].view(np.uint32))


def test_undistorter_staging_through_source_pitches(api, synth):
    rows, cols, K = 121, 333, (300.5, 301.25, 170.3, 60.7)
    D = (-0.05, 0.01, 1e-4, -5e-5)
    u = api.Undistorter(rows, cols, K, D)
    img = synth.random_image(34, rows, cols)
    ref = U.undistort(img, K, D)
    wide = np.full((rows, cols + 61), 7, np.uint8); wide[:, :cols] = img
    for src in (img, wide[:, :cols], img, wide[:, :cols]):      # src_step == cols, a wider pitch (the staging block grows), and both again
        assert np.array_equal(u.UndistortImage(src), ref), src.strides


def _tracker_round(api, pkg, synth, torch):
    case = TC.make(pkg.chain, synth, "growth", n=48)
    rows, cols = case["prev"].shape
    trk = api.Tracker(1, rows, cols, 64, 64, TC.K_of(rows, cols), 10, 4)
    trk.set_frame(0, case["st"], image=case["prev"])
    d_img = torch.from_numpy(case["cur"]).cuda(); d_res = torch.zeros(80, dtype=torch.uint8, device="cuda")
    trk.step_batch(d_img.data_ptr(), cols, rows * cols, d_res.data_ptr())
    torch.cuda.synchronize()
    post = trk.get_frame(0, image=True)
    rec = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    assert int(rec["status"][0]) >= 0 and int(rec["n_features"][0]) > 0
    return [d_res.cpu().numpy().tobytes()] + [np.asarray(post[k]).tobytes() for k in sorted(post)]


def _pnp_round(api, pkg, synth, torch):
    pw, uv, K, _, _ = synth.pnp_problem(100, 0.3, 0.5, seed=3)
    cap = 128
    p3 = np.full((1, cap, 3), np.nan, np.float32); p2 = np.full((1, cap, 2), np.nan, np.float32)
    p3[0, :100] = pw; p2[0, :100] = uv
    d3, d2 = torch.from_numpy(p3).cuda(), torch.from_numpy(p2).cuda()
    cnt = torch.full((1,), 100, dtype=torch.int32, device="cuda")
    pose = torch.zeros(7, dtype=torch.float64, device="cuda"); flag = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ninl = torch.zeros(1, dtype=torch.int32, device="cuda"); st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    solver = api.PnPSolver(1, cap)
    solver.solve_batch(d3.data_ptr(), d2.data_ptr(), cnt.data_ptr(), 1, K, pose.data_ptr(), flag.data_ptr(), ninl.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and int(ninl.item()) >= 20
    return [t.cpu().numpy().tobytes() for t in (pose, flag, ninl, st)]


def _lcddb_round(api, pkg, synth, torch):
    n0, n1 = 60, 100
    db = synth.lcd_database(n1, seed=9); ids = np.arange(n1, dtype=np.uint64) * 2 + 1
    t_db = torch.from_numpy(db).cuda()
    D = api.LoopDatabase(64)
    s = torch.cuda.Stream()
    ctx = D.context(s.cuda_stream)
    qs = np.ascontiguousarray(db[[5, 40, 17]]); cur = np.full(3, int(ids[-1]) + 40, np.uint64)
    d_q = torch.from_numpy(qs).cuda()
    out = []
    n = 0
    for upto in (n0, n1):                                    # the second append outgrows the allocation: the matrix moves under the context
        D.append_batch(ids[n:upto], t_db.data_ptr() + n * 1064 * 4, upto - n)
        n = upto
        o = (torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        ctx.query_batch(d_q.data_ptr(), cur, 3, *[t.data_ptr() for t in o])
        s.synchronize()
        assert o[0].cpu().numpy().tolist() == [int(ids[5]), int(ids[40]), int(ids[17])]
        out += [t.cpu().numpy().tobytes() for t in o] + [repr(D.query(qs[1], int(cur[0])))]
    assert len(D) == n1 and D.generation() == 1 and D.capacity() >= n1
    del ctx
    return out


@pytest.mark.parametrize("make_round", [_tracker_round, _pnp_round, _lcddb_round], ids=["tracker", "pnp", "lcddb"])
def test_create_use_destroy_three_times(api, pkg, synth, make_round):
    import torch
    rounds = [make_round(api, pkg, synth, torch) for _ in range(3)]      # every handle of a round is destroyed when the round returns
    assert rounds[0] == rounds[1] == rounds[2]


def test_loop_corrector_create_use_destroy_three_times(api, oracle, synth):
    import loop_correct_ref as R
    item = R.build_item(synth, oracle, 30, 1, 4)
    t = R.pack([item], **CAPS)
    outs = []
    for _ in range(3):
        out = Run(api, t, CAPS)()                            # its own corrector, destroyed with the Run
        assert out["status"][0] == R.DONE
        outs.append({k: np.ascontiguousarray(v).tobytes() for k, v in out.items()})
    assert outs[0] == outs[1] == outs[2]
