"""myslam_orb_process_keyframes_batch (api.ORBextractor.process_keyframes_batch): the ORB half of LoopClosing::ProcessNewKF (src/loopclosing.cpp:93-113)
for a batch of key-frames on the device, against the oracle's ScreenAndComputeKPsParams and CalcDescriptors applied to the Python expansion of
tests/test_process_kf_ref.py.  Every comparison is exact: the 28 bytes of every key-point, the 32 of every descriptor, counts and status words.

Shapes: 240 x 320, and 243 x 325 with a row pitch of 352 — the smallest at which the 8-level plan still has a FAST cell at level 7.  An image's
stride is larger than rows x pitch and every byte outside an image is 0xFF; feature slots beyond an item's count are NaN; every output buffer is
pre-filled with a sentinel and slots from the written count on must still hold it.  ORB with nfeatures = 150 (about 150 level-0 features per image),
feat_cap 192, cap 1536 unless a case says otherwise."""
import numpy as np
import pytest

from test_process_kf_ref import reference

pytestmark = pytest.mark.gpu

NF, FEAT, CAP, GAP = 150, 192, 1536, 192
SHAPES = [(240, 320, 320), (243, 325, 352)]                     # rows, cols, row pitch
KSENT, DSENT, ISENT = 0xA5, 0x5A, -7
OK, INVALID, CAPACITY, UNSUPPORTED = 0, -1, -3, -4

_cache = {}


def _image(synth, seed, rows, cols):
    key = ("img", seed, rows, cols)
    if key not in _cache:
        _cache[key] = synth.random_image(seed, rows, cols)
    return _cache[key]


def _features(oracle, img):
    """the frontend's level-0 features of an image: (n, 2) f32 pixels"""
    key = ("feat", img.tobytes())
    if key not in _cache:
        f = oracle.detect(oracle.params(NF), img)
        _cache[key] = np.stack([f["x"], f["y"]], 1).astype(np.float32)
    return _cache[key]


def _want(oracle, img, xy):
    key = ("ref", img.tobytes(), np.asarray(xy, np.float32).tobytes())
    if key not in _cache:
        _cache[key] = reference(oracle, oracle.params(NF), img, np.asarray(xy, np.float32).reshape(-1, 2))
    return _cache[key]


def _per_level(kps):
    return [int((kps["octave"] == l).sum()) for l in range(8)]


class Call:
    """the device buffers of one call: images at `step` / stride rows * step + GAP inside 0xFF, NaN beyond an item's features, sentinels in every output"""

    def __init__(self, torch, api, imgs, step, xys, n_feat=None, feat_cap=FEAT, cap=CAP):
        self.torch, self.api = torch, api
        self.B, (self.rows, self.cols), self.step, self.feat_cap, self.cap = len(imgs), imgs[0].shape, step, feat_cap, cap
        self.stride = self.rows * step + GAP
        self.d_imgs = torch.empty(self.B * self.stride, dtype=torch.uint8, device="cuda")
        self.d_xy = torch.empty(self.B * feat_cap * 2, dtype=torch.float32, device="cuda")
        self.d_n = torch.empty(self.B, dtype=torch.int32, device="cuda")
        self.d_kps = torch.empty(self.B * cap * 28, dtype=torch.uint8, device="cuda")
        self.d_desc = torch.empty(self.B * cap * 32, dtype=torch.uint8, device="cuda")
        self.d_cnt = torch.empty(self.B, dtype=torch.int32, device="cuda")
        self.d_st = torch.empty(self.B, dtype=torch.int32, device="cuda")
        self.load(imgs, xys, n_feat)
        self.clear()

    def load(self, imgs, xys, n_feat=None):
        host = np.full((self.B, self.stride), 0xFF, np.uint8)
        xy = np.full((self.B, self.feat_cap, 2), np.nan, np.float32)
        for b, (img, pts) in enumerate(zip(imgs, xys)):
            host[b, :self.rows * self.step].reshape(self.rows, self.step)[:, :self.cols] = img
            pts = np.asarray(pts, np.float32).reshape(-1, 2)[:self.feat_cap]
            xy[b, :len(pts)] = pts
        self.d_imgs.copy_(self.torch.from_numpy(host.ravel()))
        self.d_xy.copy_(self.torch.from_numpy(xy.ravel()))
        self.d_n.copy_(self.torch.from_numpy(np.asarray([len(p) for p in xys] if n_feat is None else n_feat, np.int32)))

    def clear(self):
        self.d_kps.fill_(KSENT); self.d_desc.fill_(DSENT); self.d_cnt.fill_(ISENT); self.d_st.fill_(ISENT)

    def args(self, **kw):
        a = dict(d_imgs=self.d_imgs.data_ptr(), batch=self.B, rows=self.rows, cols=self.cols, step=self.step, img_stride=self.stride,
                 d_feat_xy=self.d_xy.data_ptr(), d_n_feat=self.d_n.data_ptr(), feat_cap=self.feat_cap, d_pyr_kps=self.d_kps.data_ptr(),
                 d_desc=self.d_desc.data_ptr(), d_counts=self.d_cnt.data_ptr(), d_status=self.d_st.data_ptr(), cap=self.cap)
        a.update(kw)
        return a

    def run(self, ext, **kw):
        ext.process_keyframes_batch(**self.args(**kw))

    def results(self):
        self.torch.cuda.synchronize()
        return dict(kps=self.d_kps.cpu().numpy().reshape(self.B, self.cap * 28), desc=self.d_desc.cpu().numpy().reshape(self.B, self.cap, 32),
                    cnt=self.d_cnt.cpu().numpy(), st=self.d_st.cpu().numpy())

    def untouched(self):
        r = self.results()
        return (r["kps"] == KSENT).all() and (r["desc"] == DSENT).all() and (r["cnt"] == ISENT).all() and (r["st"] == ISENT).all()


def _check_item(r, b, want, tag=""):
    wk, wd = want
    n = len(wk)
    assert (int(r["cnt"][b]), int(r["st"][b])) == (n, OK), (tag, b, int(r["cnt"][b]), int(r["st"][b]), n)
    got = r["kps"][b, :n * 28].copy().view(wk.dtype)
    assert got.tobytes() == wk.tobytes(), (tag, b, [f for f in wk.dtype.names if not np.array_equal(got[f].view(np.int32), wk[f].view(np.int32))])
    assert np.array_equal(r["desc"][b, :n], wd), (tag, b, int((r["desc"][b, :n] != wd).any(1).sum()))
    assert (r["kps"][b, n * 28:] == KSENT).all() and (r["desc"][b, n:] == DSENT).all(), (tag, b, "slots beyond the count were written")


def _ext(api, torch, stream=None):
    ext = api.ORBextractor(NF)
    ext.set_stream((stream or torch.cuda.current_stream()).cuda_stream)
    return ext


def _parity_items(oracle, synth, rows, cols):
    """n_feat = 0, 1, 61, all of them, feat_cap + 7 (the item's slots filled up to feat_cap), and a constant image with 50 features"""
    imgs = [_image(synth, 800 + i, rows, cols) for i in range(5)] + [np.full((rows, cols), 128, np.uint8)]
    rng = np.random.default_rng(rows)
    rand = lambda n: np.stack([rng.uniform(0, cols, n), rng.uniform(0, rows, n)], 1).astype(np.float32)
    f = [_features(oracle, im) for im in imgs[:5]]
    xys = [f[0][:0], f[1][:1], f[2][:61], f[3], np.concatenate([f[4], rand(FEAT)])[:FEAT], rand(50)]
    n_feat = [0, 1, 61, len(f[3]), FEAT + 7, 50]
    return imgs, xys, n_feat


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("rows,cols,step", SHAPES)
def test_parity_with_the_oracle(api, oracle, synth, rows, cols, step):
    import torch
    imgs, xys, n_feat = _parity_items(oracle, synth, rows, cols)
    want = [_want(oracle, im, xy) for im, xy in zip(imgs, xys)]
    # the input is not degenerate (the oracle's output alone): every level keeps and drops rows; level 0 of an unblurred image drops none, since
    # its features ARE its FAST corners
    kept = _per_level(want[3][0])
    assert 140 <= len(xys[3]) <= FEAT and kept[0] == len(xys[3]) and all(0 < k < len(xys[3]) for k in kept[1:]), kept
    assert len(xys[4]) == FEAT and len(want[5][0]) == 0 and len(want[0][0]) == 0 and 1 <= len(want[1][0]) <= 8
    c = Call(torch, api, imgs, step, xys, n_feat)
    ext = _ext(api, torch)
    for rep in range(2):                                             # twice: the scratch is reused
        c.clear(); c.run(ext)
        r = c.results()
        for b in range(c.B):
            _check_item(r, b, want[b], rep)


# ------------------------------------------------------------------------------------------ 2. edge coordinates
def _edge_points(oracle, rows, cols):
    """for l = 0, 3, 7 and both axes: 19 * scale[l], the float just below it, (w_l - 19) * scale[l], the float just below it — each beside six
    values of the other coordinate, so that some of the points sit on a FAST corner of the level; then NaN, +-inf, -5 and 1e9 on either axis"""
    sc, isc = oracle.orb_tables(oracle.params(NF))[:2]
    pts, tags = [], []
    below = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    bases = [np.asarray([cols * (0.2 + 0.1 * j) + 0.25, rows * (0.2 + 0.1 * j) - 0.25], np.float32) for j in range(6)]
    for l in (0, 3, 7):
        dims = oracle.level_size(cols, rows, float(isc[l]))
        for axis in (0, 1):
            lo, hi = np.float32(19) * sc[l], np.float32(dims[axis] - 19) * sc[l]
            for which, v in enumerate((lo, below(lo), hi, below(hi))):
                for base in bases:
                    p = base.copy(); p[axis] = v
                    pts.append(p); tags.append((l, axis, which))
    for axis in (0, 1):
        for v in (np.nan, np.inf, -np.inf, -5.0, 1e9):
            p = bases[2].copy(); p[axis] = v
            pts.append(p); tags.append(None)
    return np.asarray(pts, np.float32), tags


def test_edge_coordinates(api, oracle, synth):
    import torch
    rows, cols, step = SHAPES[1]
    img = _image(synth, 811, rows, cols)
    edge, tags = _edge_points(oracle, rows, cols)
    xy = np.concatenate([edge, _features(oracle, img)])[:FEAT]
    assert len(edge) == 154 and len(xy) == FEAT
    wk, wd = _want(oracle, img, xy)
    # on the oracle: at every one of the three levels and on both axes a point at 19 * scale is kept (it sits on a corner for some base) and none
    # just below it is; the upper border keeps some and drops some; the non-finite and far points keep nothing
    kept = {}
    for i, t in enumerate(tags):
        if t is not None:
            kept[t] = kept.get(t, 0) + int(((wk["class_id"] == i) & (wk["octave"] == t[0])).any())
    for l in (0, 3, 7):
        for axis in (0, 1):
            assert kept[(l, axis, 0)] >= 1 and kept[(l, axis, 1)] == 0, (l, axis, kept)
    upper = [kept[(l, axis, w)] for l in (0, 3, 7) for axis in (0, 1) for w in (2, 3)]
    assert any(upper) and not all(upper), kept
    assert not np.isin(wk["class_id"], [i for i, t in enumerate(tags) if t is None]).any()
    # a kept row shows the bits (pt / scale) * scale left, not the caller's
    moved = (wk["x"].view(np.int32) != xy[wk["class_id"], 0].view(np.int32)) | (wk["y"].view(np.int32) != xy[wk["class_id"], 1].view(np.int32))
    assert moved.any() and not moved.all()
    c = Call(torch, api, [img], step, [xy])
    c.run(_ext(api, torch))
    _check_item(c.results(), 0, (wk, wd))


# ------------------------------------------------------------------------------------------ 3. batch equals single
def test_batch_equals_single_and_the_host_calls(api, oracle, synth):
    import torch
    rows, cols, step = SHAPES[1]
    imgs, xys, n_feat = _parity_items(oracle, synth, rows, cols)
    c = Call(torch, api, imgs, step, xys, n_feat)
    ext = _ext(api, torch)
    c.run(ext)
    r = c.results()
    from test_process_kf_ref import expand
    for b in (2, 3, 4):
        one = Call(torch, api, [imgs[b]], step, [xys[b]], [n_feat[b]])
        one.run(ext)
        q = one.results()
        n = int(q["cnt"][0])
        assert n == int(r["cnt"][b]) > 0 and q["st"][0] == r["st"][b] == OK
        assert np.array_equal(q["kps"][0], r["kps"][b]) and np.array_equal(q["desc"][0], r["desc"][b])
        kout, _ = ext.ScreenAndComputeKPsParams(imgs[b], expand(api.KP_DTYPE, xys[b]))          # the host-pointer path of the same build
        assert kout.tobytes() == r["kps"][b, :n * 28].tobytes()
        assert np.array_equal(ext.CalcDescriptors(imgs[b], kout), r["desc"][b, :n])


# ------------------------------------------------------------------------------------------ 4. after the in-place blur
def test_after_the_deeplcd_blur_in_place(api, oracle, synth):
    import torch
    rows, cols, step = SHAPES[0]
    imgs = [_image(synth, 800 + i, rows, cols) for i in range(2)]
    xys = [_features(oracle, im) for im in imgs]
    blurred = [oracle.calc_preproc(im, blur_in_place=True)[1] for im in imgs]
    want = [_want(oracle, bl, xy) for bl, xy in zip(blurred, xys)]
    kept = _per_level(want[0][0])
    assert all(0 < k < len(xys[0]) for k in kept), kept             # the blur removes corners at level 0 too
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lcd = api.DeepLCD(synth.calc_weights(), stream=s.cuda_stream)
        ext = _ext(api, torch, s)
        c = Call(torch, api, imgs, step, xys)
        alone = Call(torch, api, imgs, step, xys)
        d_out = torch.zeros(2, 1064, device="cuda"); d_alone = torch.zeros(2, 1064, device="cuda")
        lcd.describe_batch(alone.d_imgs.data_ptr(), 2, rows, cols, step, alone.stride, d_alone.data_ptr(), blur_in_place=True)
        lcd.describe_batch(c.d_imgs.data_ptr(), 2, rows, cols, step, c.stride, d_out.data_ptr(), blur_in_place=True)
        c.run(ext)                                                  # same stream, nothing in between
        r = c.results()
    for b in range(2):
        _check_item(r, b, want[b])
    assert torch.equal(c.d_imgs, alone.d_imgs) and torch.equal(d_out.view(torch.int32), d_alone.view(torch.int32))
    got = c.d_imgs.cpu().numpy()[:rows * step].reshape(rows, step)[:, :cols]
    assert np.array_equal(got, blurred[0])


# ------------------------------------------------------------------------------------------ 5. capacity and arguments
def test_capacity_and_arguments(api, oracle, synth):
    import torch
    rows, cols, step = SHAPES[0]
    imgs = [_image(synth, 800 + i, rows, cols) for i in range(3)]
    f = [_features(oracle, im) for im in imgs]
    xys = [f[0][:61], f[1], f[2][:61]]
    want = [_want(oracle, im, xy) for im, xy in zip(imgs, xys)]
    n1 = len(want[1][0])
    assert max(len(want[0][0]), len(want[2][0])) < n1 - 1
    ext = _ext(api, torch)
    exact = Call(torch, api, imgs, step, xys, cap=n1)               # a cap that just holds the item
    exact.run(ext)
    r = exact.results()
    for b in range(3):
        _check_item(r, b, want[b], "cap = count")
    c = Call(torch, api, imgs, step, xys, cap=n1 - 1)
    c.run(ext)
    r = c.results()
    assert (int(r["cnt"][1]), int(r["st"][1])) == (0, CAPACITY)
    assert (r["kps"][1] == KSENT).all() and (r["desc"][1] == DSENT).all()
    _check_item(r, 0, want[0]); _check_item(r, 2, want[2])
    # call level: nothing is enqueued, nothing written
    c.clear()
    bad = [dict(d_imgs=0), dict(d_feat_xy=0), dict(d_n_feat=0), dict(d_pyr_kps=0), dict(d_desc=0), dict(d_counts=0), dict(d_status=0),
           dict(batch=0), dict(batch=-1), dict(rows=0), dict(cols=0), dict(cols=-3), dict(feat_cap=0), dict(cap=0), dict(cap=-1), dict(step=cols - 1)]
    for kw in bad:
        with pytest.raises(api.MyslamError) as e:
            c.run(ext, **kw)
        assert e.value.code == INVALID, kw
    a = c.args()
    assert api.lib().myslam_orb_process_keyframes_batch(None, *[a[k] for k in a]) == INVALID
    with pytest.raises(api.MyslamError) as e:                       # no FAST grid fits a 40 x 40 image
        c.run(ext, rows=40, cols=40, step=40, img_stride=1600)
    assert e.value.code == UNSUPPORTED
    assert c.untouched()
    c.run(ext)                                                      # the handle is as good as before
    r = c.results()
    assert (int(r["cnt"][1]), int(r["st"][1])) == (0, CAPACITY)
    _check_item(r, 0, want[0]); _check_item(r, 2, want[2])


# ------------------------------------------------------------------------------------------ 6. feeds the matcher
def test_output_feeds_loop_match_batch(api, oracle, synth):
    import torch
    rows, cols, step = SHAPES[0]
    loop_img = _image(synth, 800, rows, cols)
    cur_img = np.roll(loop_img, 2, axis=1)                          # the current key-frame sees the loop key-frame's scene 2 pixels to the right
    loop_xy = _features(oracle, loop_img)
    cur_xy = loop_xy + np.asarray([2, 0], np.float32)
    (lk, ld), (ck, cd) = _want(oracle, loop_img, loop_xy), _want(oracle, cur_img, cur_xy)
    ti, dist = oracle.hamming_match(ld, cd)                         # query = loop, train = current (loopclosing.cpp:172)
    lim = max(2.0 * float(dist.min()), 30.0)
    pairs = sorted(set((int(ck["class_id"][t]), int(lk["class_id"][i])) for i, (t, d) in enumerate(zip(ti, dist)) if float(d) <= lim))
    assert len(pairs) >= 10 and len(lk) > 300 and len(ck) > 300
    ext = _ext(api, torch)
    loop = Call(torch, api, [loop_img], step, [loop_xy]); cur = Call(torch, api, [cur_img], step, [cur_xy])
    loop.run(ext); cur.run(ext)
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device="cuda")
    d_lm = i32(FEAT, -1); d_pos = torch.zeros(3, dtype=torch.float64, device="cuda")
    d_ti, d_dist, d_pairs, d_np, d_valid = i32(CAP, ISENT), i32(CAP, ISENT), i32(CAP * 2, ISENT), i32(1, ISENT), i32(64 * 2, ISENT)
    d_p3 = torch.zeros(64 * 3, device="cuda"); d_p2 = torch.zeros(64 * 2, device="cuda"); d_cnt = i32(1, ISENT); d_st = i32(1, ISENT)
    # the two calls' output buffers go straight in: no host copy in between
    api.loop_match_batch(loop.d_desc.data_ptr(), loop.d_cnt.data_ptr(), cur.d_desc.data_ptr(), cur.d_cnt.data_ptr(), loop.d_kps.data_ptr(),
                         cur.d_kps.data_ptr(), 1, CAP, cur.d_xy.data_ptr(), d_lm.data_ptr(), FEAT, d_pos.data_ptr(), 0, 1, 10, 64, d_ti.data_ptr(),
                         d_dist.data_ptr(), d_pairs.data_ptr(), d_np.data_ptr(), d_valid.data_ptr(), d_p3.data_ptr(), d_p2.data_ptr(), d_cnt.data_ptr(),
                         d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = len(lk)
    assert int(loop.d_cnt.item()) == n and int(cur.d_cnt.item()) == len(ck)
    assert np.array_equal(d_ti.cpu().numpy()[:n], ti) and np.array_equal(d_dist.cpu().numpy()[:n], dist)
    assert (d_ti.cpu().numpy()[n:] == ISENT).all() and (d_dist.cpu().numpy()[n:] == ISENT).all()
    assert int(d_np.item()) == len(pairs)
    assert d_pairs.cpu().numpy().reshape(-1, 2)[:len(pairs)].tolist() == [list(p) for p in pairs]
    assert int(d_st.item()) == 2 and int(d_cnt.item()) == 0         # no loop feature has a map point here: MYSLAM_LOOP_MATCH_FEW_POINTS


# ------------------------------------------------------------------------------------------ 7. recorded step
def test_recorded_step_reads_the_buffers_of_the_replay(api, oracle, synth):
    import torch
    rows, cols, step = SHAPES[1]
    A = [_image(synth, 800 + i, rows, cols) for i in range(2)]
    Bi = [_image(synth, 802 + i, rows, cols) for i in range(2)]
    xa = [_features(oracle, im) for im in A]
    xb = [_features(oracle, im)[::-1][:100 + 20 * i] for i, im in enumerate(Bi)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ext = _ext(api, torch, s)
        c = Call(torch, api, A, step, xa)
        c.run(ext)                                                  # eager: the lazy allocations happen here
        first = c.results()
        c.load(Bi, xb); c.clear(); c.run(ext)
        want = c.results()
        assert not np.array_equal(first["cnt"], want["cnt"])
        c.load(A, xa); c.clear()
        torch.cuda.synchronize()
        g = api.StepGraph.record(s.cuda_stream, [], lambda: c.run(ext))
        assert g.node_count() >= 4                                  # pyramid, Gaussian, screen, compaction, descriptors
        assert c.untouched(), "recording a step must not run it"
        c.load(Bi, xb)
        g.launch(s.cuda_stream)
        got = c.results()
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        c.load(A, xa); c.clear()
        g.launch(s.cuda_stream)
        got = c.results()
        for k in first:
            assert np.array_equal(got[k], first[k]), k
    for b in range(2):
        _check_item(want, b, _want(oracle, Bi[b], xb[b]))


# ------------------------------------------------------------------------------------------ 8. shared handle
def test_shared_handle_leaves_the_other_calls_alone(api, oracle, synth):
    import torch
    rows, cols, step = SHAPES[0]
    imgs = np.stack([_image(synth, 800 + i, rows, cols) for i in range(3)])
    xys = [_features(oracle, im) for im in imgs[:2]]
    d_imgs = torch.from_numpy(imgs).cuda()

    def dac(ext):
        cap = ext.max_keypoints(rows, cols)
        k = torch.full((3 * cap * 28,), KSENT, dtype=torch.uint8, device="cuda"); d = torch.full((3 * cap * 32,), DSENT, dtype=torch.uint8, device="cuda")
        n = torch.full((3,), ISENT, dtype=torch.int32, device="cuda"); st = torch.full((3,), ISENT, dtype=torch.int32, device="cuda")
        ext.detect_and_compute_batch(d_imgs.data_ptr(), 3, rows, cols, cols, rows * cols, k.data_ptr(), d.data_ptr(), n.data_ptr(), st.data_ptr(), cap)
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (k, d, n, st)]

    def pkf(ext):
        c = Call(torch, api, list(imgs[:2]), step, xys)
        c.run(ext)
        return c.results()

    def host(ext):
        k, d = ext.DetectAndCompute(imgs[2])
        return [k.tobytes(), d.tobytes()]

    shared = _ext(api, torch)
    got = [dac(shared), pkf(shared), dac(shared), host(shared), pkf(shared), host(shared)]
    fresh = _ext(api, torch)
    want = [dac(fresh), None, dac(fresh), host(fresh), None, host(fresh)]
    alone = pkf(_ext(api, torch))
    for i in (0, 2, 3, 5):
        assert got[i] == want[i], i
    for i in (1, 4):
        for k in alone:
            assert np.array_equal(got[i][k], alone[k]), (i, k)
    for b in range(2):
        _check_item(alone, b, _want(oracle, imgs[b], xys[b]))
    rk, rd = oracle.detect_and_compute(oracle.params(NF), imgs[2])
    assert got[3] == [rk.tobytes(), rd.tobytes()]
